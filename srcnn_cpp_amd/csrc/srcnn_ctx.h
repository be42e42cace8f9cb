// srcnn_ctx.h -- what the host-side translation units of the C-ABI layer share: the context, error / device-scope helpers and
// the declarations of the functions that cross a file boundary.  Not installed; the public boundary is include/srcnn_amd.h.
//   srcnn_api.cpp     context life cycle, modes, streams, device memory, the REFBYTES monitor's entry points
//   srcnn_model.cpp   weight tables: power-of-two layer scales, MFMA fragment packers, split-f16 ranges, the flag threshold
//   srcnn_plan.cpp    launch geometry: regular grid, balanced work items and seams, item-table cache, srcnn_query_plan
//   srcnn_launch.cpp  run_strip() -- the one launch path of the strip kernels and the fix-up -- and the device-pointer entry points
//   srcnn_host.cpp    host-buffer entry points: staging, band / frame pipelines, the reference call surface, the pipeline steps
//   srcnn_multi.cpp   several GPUs from one host process: row-striped plane, frame ranges
//   srcnn_spatial.cpp the banded path (9-3-5 / 9-5-5, zero padding, colour models): weight table, gate, band loop, entry points
//   srcnn_resize_f32.cpp the cubic resize of float32 planes in front of the float image path: tap tables, entry points, and a
//                     3-plane float image through a 1-channel model (srcnn_process_rgb_f32*)
#pragma once
#include "../../include/srcnn_amd.h"
#include "srcnn_kernels.h"

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

// Experiment knobs (SRCNN_DEBUG_*, SRCNN_HOST_COPY_THREADS) and the srcnn_debug_* test hooks exist only in the TUNING build of
// the library (-DSRCNN_TUNING_BUILD: libsrcnn_amd_tuning.so, which tools/ and the tests that need the hooks load by path).
// The product library reads no environment variable and exports exactly the symbols of include/srcnn_amd.h
// (tests/test_abi.py checks both on the built file).
#ifdef SRCNN_TUNING_BUILD
#define SRCNN_DEBUG_ENV(name) std::getenv(name)
#else
#define SRCNN_DEBUG_ENV(name) static_cast<const char *>(nullptr)
#endif

namespace srcnn {
namespace host {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

// Persistent host threads of the several-GPUs entry points (srcnn_forward_y_striped*, srcnn_forward_y_frames_multi):
// one worker per context beyond the first, created on first use and parked on a condition variable between calls.
// Spawning and joining n_ctx - 1 std::threads PER STEP cost tens of microseconds next to 0.47 ms of kernel per rank for
// a 7680x4320 plane on 8 GPUs.  Owned by the first context of the set (a context belongs to one host thread at a time,
// include/srcnn_amd.h), destroyed with it.
class WorkerPool {
    struct Worker {
        std::thread th;
        std::mutex m;
        std::condition_variable cv;
        std::function<int()> task;
        bool has_task = false, done = false, stop = false;
        int rc = 0;
    };
    std::vector<std::unique_ptr<Worker>> workers_;

    static void loop(Worker *w)
    {
        std::unique_lock<std::mutex> lk(w->m);
        for (;;) {
            w->cv.wait(lk, [w] { return w->has_task || w->stop; });
            if (w->stop) return;
            std::function<int()> t = std::move(w->task);
            w->has_task = false;
            lk.unlock();
            const int rc = t();
            lk.lock();
            w->rc = rc;
            w->done = true;
            w->cv.notify_all();
        }
    }

public:
    WorkerPool() = default;
    WorkerPool(const WorkerPool &) = delete;
    WorkerPool &operator=(const WorkerPool &) = delete;
    ~WorkerPool()
    {
        for (auto &w : workers_) {
            { std::lock_guard<std::mutex> lk(w->m); w->stop = true; }
            w->cv.notify_all();
            if (w->th.joinable()) w->th.join();
        }
    }
    // fn(k) for k = 0 .. n - 1: k = 0 on the calling thread, the others on the parked workers; returns the first non-zero code.
    // Every missing worker is created BEFORE any task is posted, and nothing is thrown to the caller (the C ABI sits right
    // above): a thread or an allocation that cannot be had returns `nomem` with no task started -- no worker is left running a
    // task that refers to this frame.
    // `on_incomplete` runs when not every task could be started (the tasks that WERE started are still waited for): a set of
    // tasks that wait for each other -- the striped-frames pipeline -- must learn that some of them will never run.
    template <typename Fn>
    int run(int n, Fn fn, int nomem = SRCNN_ERR_NOMEM) { return run(n, fn, nomem, [] {}); }
    template <typename Fn, typename Abort>
    int run(int n, Fn fn, int nomem, Abort on_incomplete)
    {
        try {
            while ((int)workers_.size() < n - 1) {
                std::unique_ptr<Worker> w(new Worker());
                w->th = std::thread(loop, w.get());
                workers_.push_back(std::move(w));
            }
        } catch (...) {
            return nomem;
        }
        int posted = 0, first = 0;
        try {
            for (int k = 1; k < n; ++k) {
                Worker *w = workers_[(size_t)k - 1].get();
                { std::lock_guard<std::mutex> lk(w->m); w->task = [&fn, k] { return fn(k); }; w->has_task = true; w->done = false; }
                w->cv.notify_all();
                posted = k;
            }
            first = fn(0);
        } catch (...) {
            first = nomem;             // (std::function may allocate; fn itself is this library's code and does not throw)
            on_incomplete();
        }
        for (int k = 1; k <= posted; ++k) {       // whatever happened above, every posted task is waited for before this frame goes
            Worker *w = workers_[(size_t)k - 1].get();
            std::unique_lock<std::mutex> lk(w->m);
            w->cv.wait(lk, [w] { return w->done; });
            if (!first && w->rc) first = w->rc;
        }
        return first;
    }
    int size() const { return (int)workers_.size(); }
};

}  // namespace host
}  // namespace srcnn

// SRCNN_MODE_REFBYTES: default factor of the flag threshold's weight-proportional term (fixup_delta(), srcnn_set_fixup_margin)
constexpr float kFixMargin = 4.f;
// ... its absolute term (roundings at the output's own magnitude: fixup_delta()).
// The PER-PIXEL threshold (round 6; srcnn_set_fixup_local):  thr(x) = min(delta, margin * kFixLocal * 2^-24 * S1(x) + kFixAbsLocal),
// S1 = the pixel's local scale (srcnn_kernels.h, l3_row_is_scale()).  How (k, abs) = (4 * kFixLocal, kFixAbsLocal) were chosen
// (profiles/r06/README.md, "the per-pixel threshold"): the noise has a part that does not shrink with S1 -- with abs = 6.1e-5 the
// windows of small local scale ask for k = 2.4, with 2.44e-4 for 1.48 -- and among the pairs that keep
//   (R1) thr >= 1.73 x the deviation of EVERY window an adversarial search has produced (the factor the global delta keeps over the
//        worst of them), the searches climbing on exactly that quantity: 241 M and, from another seed, 906 M point evaluations on the CPU models
//        (fixup_adversarial_ratio.txt: k >= 1.480, _long.txt: 1.540; random models <= 1.05), 5.2 M window evaluations on the kernel itself in two
//        independent climbs (adversarial_gpu_ratio.txt: 1.480, adversarial_gpu_ratio_long.txt: 1.525; split-f16 kernel: 2.023 both), and
//   (R2) thr >= 2.5 x the largest deviation on content (it then stays below 0.4 thr, short of the 1/2 at which the device-side net
//        redoes a launch): 1.485 (sparse bright strokes on a dark ground; split-f16 kernel: 1.777),
// abs = 16 * 2^-24 * 256 = 2.44e-4 is the cheapest on ordinary content.  k = 1.6 / 2.15 keep 4-6 % over the largest of those figures.
constexpr float kFixAbsTerm = 4.f * 256.f / 16777216.f;
constexpr float kFixAbsLocal = 16.f * 256.f / 16777216.f;
constexpr float kFixLocal = 0.4f;
constexpr float kFixLocal16 = 0.5375f;     // SRCNN_MODE_REFBYTES16: the split-f16 kernel's noise is wider (k = 2.15)

struct srcnn_ctx {
    int device = 0;
    int n_cu = 256;
    int mode = SRCNN_MODE_MFMA;
    bool safe_hazards = false;             // launch the hazard-safe strip kernels (the interlock probe failed on this device)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    char err[512] = "no error";
    // model
    bool has_l12 = false, has_l3 = false;   // which layers of the uploaded tables came from the caller (the rest are zeros)
    float b3 = 0.f;
    srcnn::host::DevBuf wfrag;   // packed MFMA fragments [NFRAG][64]
    srcnn::host::DevBuf wfrag16; // split-f16 fragments (SRCNN_MODE_SPLIT16), S16_TABLE_BYTES
    bool split16_ok = false;   // the uploaded weights fit the f16 ranges of that mode (split16_range_ok)
    srcnn::host::DevBuf wraw;    // b1|W1|b2|W2|b3|W3 in convdata.h order (exact kernels)
    // The banded path (srcnn_spatial.cpp): every model but a 1-channel 9-1-5 one under replicate padding.  channels, f2: the
    // loaded model (a colour model: channels = 3, and the 9-1-5 tables hold a zero model that no gate lets run, luma_path_ok).
    // Layers 1-3 run from sp_table (spatial_table_floats(channels, f2)) with the biases sp_b3, packed for the model with layer 2
    // sp_f2: srcnn_set_model (f2 > 1) and srcnn_set_model_color pack them when they load, a 9-1-5 model is packed from host_raw
    // the first time a zero-padded call needs it (sp_f2 = 0: nothing packed since the last upload_weights).  A 1-channel f2 > 1
    // model under replicate padding runs layer 3 on MODE_L3 from wfrag / b3, which srcnn_set_model loads with W2 = 0.  The two
    // maps of one row band, and the event behind the last launch that used them (so that launches on another stream -- the frame
    // lanes -- wait before reusing them).
    int channels = 1;
    int f2 = 1;
    // The widths of the loaded model (srcnn_set_model_shape): n1 / n2 filters as given, n1p / n2p padded with zero channels to a
    // multiple of 64 / 32.  64 / 32 for every model the other loaders load.  A WIDE model (n1p = 128 or n2p = 64, wide_model())
    // lives in sp_table alone, spatial_table_floats() of its widths (srcnn_kernels.h), and sp_map64 / sp_map32 hold n1p / n2p
    // planes; it runs in SRCNN_MODE_MFMA through forward_banded() and nowhere else.
    int n1 = 64, n2 = 32, n1p = 64, n2p = 32;
    // srcnn_set_wide_split16: a setting of the context like the padding (kept across model loads).  1: forward_banded() runs
    // layer 2 of a WIDE model in split f16 (spatial_l2h_kernel's wide forms), from the sp16_* state below made for n1p / n2p; a narrow
    // model ignores it.
    int wide_split16 = 0;
    srcnn::host::DevBuf sp_table, sp_map64, sp_map32;
    float sp_b3[3] = {0.f, 0.f, 0.f};
    int sp_f2 = 0;
    // SRCNN_MODE_BANDED16 (layer 2 in split f16): a host copy of W2 [32][64][sp_f2][sp_f2] and the bound of the layer-1 map for
    // 8-bit input, max_k (255 sum |w1[k]| + |b1[k]|), both kept by upload_table; the split W2 table (srcnn_kernels.h) and the
    // two power-of-two scales are made from them the first time a call in that mode runs the model (sp16_f2 = 0: not made since
    // the model was loaded; -1: the model cannot be scaled, the mode refuses it).  A wide model keeps the same for
    // srcnn_set_wide_split16: the padded W2 [n2p][n1p][sp_f2][sp_f2], the bound over its n1p channels, the table of
    // spatial_l2h_table_bytes() for its widths.
    std::vector<float> sp_w2;
    double sp_l1_bound = 0.0;
    srcnn::host::DevBuf sp16_table;
    int sp16_f2 = 0;
    float sp16_scale1 = 1.f, sp16_unscale = 1.f;
    // The float image path (srcnn_forward_f32*) in SRCNN_MODE_BANDED16 bounds the layer-1 map by input_range (srcnn_set_input_range,
    // a setting of the context like the padding: default 255, kept across model loads) instead of 255: upload_table keeps
    // sum |w1[k]| and |b1[k]| per layer-1 channel, upload_table16 the exponent of W2's scale, and a float call makes its two
    // scales from them.  The W2 table does not depend on the range; the byte entry points keep sp16_scale1 / sp16_unscale.
    float input_range = 255.f;
    double sp_l1_sum[128] = {}, sp_l1_absb[128] = {};      // (the first n1p of them)
    int sp16_e2 = 0;
    hipEvent_t sp_done = nullptr;
    hipStream_t sp_stream = nullptr;
    // SRCNN_PAD_ZERO (srcnn_set_padding): every model runs the banded path with the zero-padding kernels.  whole_model: the
    // tables came from srcnn_set_weights / srcnn_set_model(_color), not from per-filter calls
    int padding = SRCNN_PAD_REPLICATE;
    bool whole_model = false;
    bool per_filter = false;     // inside srcnn_conv99x11 / srcnn_conv55 on host planes (luma_path_ok)
    // staging for the host-buffer entry points
    srcnn::host::DevBuf in_u8, out_u8, pre_f32, planes, plane1, kern, sink;
    // seam scratch (srcnn_kernels.h) is written by one launch and read by the seam kernel behind it: one buffer per
    // stream the context launches on (its own, the two frame lanes, a caller's), so launches on different
    // streams never share it
    struct SeamScratch {
        hipStream_t stream = nullptr;
        bool used = false;
        srcnn::host::DevBuf buf, cbuf;           // row seams, column seams
        srcnn::host::DevBuf buf2, cbuf2;         // ... the second set of seam deferral (launches alternate: `flip`)
        int flip = 0;
        srcnn::host::DevBuf flag, fix_lists, fix_counters;     // SRCNN_MODE_REFBYTES: flag plane, work lists, per-launch counters
    };
    SeamScratch seam_scratch[4];
    // pipeline steps around the conv path
    srcnn::host::DevBuf bgr_in, bgr_out, ycc_lo, ycc_hi, y_sr, tables;
    int tab_sw = 0, tab_sh = 0, tab_dw = 0, tab_dh = 0;   // geometry the uploaded cubic tables are for
    // The float32 cubic resize (srcnn_resize_cubic_f32*, srcnn_process_f32*): the tables of one geometry and the stream of the
    // last launch that read them (ensure_tables_f32), the staging of the host-memory forms, and the one-frame workspace of
    // srcnn_process_f32* (channels x dst_w x dst_h floats, grown on demand) and of srcnn_process_rgb_f32* (two planes: Yup, Ysr)
    srcnn::host::DevBuf f32_tables, f32_lo, f32_hi, f32_work;
    int ftab_sw = 0, ftab_sh = 0, ftab_dw = 0, ftab_dh = 0;
    hipStream_t ftab_stream = nullptr;
    // The antialiased cubic resize (srcnn_resize_cubic_aa_*): the tables of one geometry with their largest tap counts, the
    // workspace of the general form (n_planes x src_h x dst_w floats, grown on demand), and the stream of the last launch that
    // used either (ensure_tables_aa, resample_aa_dev)
    srcnn::host::DevBuf aa_tables, aa_work;
    int atab_sw = 0, atab_sh = 0, atab_dw = 0, atab_dh = 0, atab_kx = 0, atab_ky = 0;
    hipStream_t aa_stream = nullptr;
    // Pillow's resize of uint8 images (srcnn_resize_pil_image_dev): a cache slot of its own -- the int32 tables of one geometry
    // and filter with their largest tap counts and the rows a tile spans, the byte workspace of the general form (n_planes x
    // src_h x dst_w, grown on demand), the planar uint8 image the process calls resize into (srcnn_process_pil_image_dev), and
    // the stream of the last launch that used any of them (ensure_tables_pil, resample_pil_dev)
    srcnn::host::DevBuf pil_tables, pil_work, pil_image;
    int ptab_sw = 0, ptab_sh = 0, ptab_dw = 0, ptab_dh = 0, ptab_filter = 0, ptab_kx = 0, ptab_ky = 0, ptab_span = 0;
    hipStream_t pil_stream = nullptr;
    // The metrics (srcnn_metrics_image_dev): the per-workgroup partial sums of one call (grown on demand) and the stream of the
    // last launch that wrote them
    srcnn::host::DevBuf metric_work;
    hipStream_t metric_stream = nullptr;
    // MS-SSIM (srcnn_msssim_image_dev): the float64 planes of the scales >= 1 and the per-workgroup partial sums of one call, in
    // one buffer (grown on demand), and the stream of the last launch that wrote it
    srcnn::host::DevBuf msssim_work;
    hipStream_t msssim_stream = nullptr;
    // second lane of the host-frame pipeline (srcnn_forward_y_frames)
    // explicit work items of single-round launches (build_items): a small cache of device tables, one per
    // launch geometry, so that a caller alternating between a few plane sizes never waits for an upload
    struct ItemTable {
        int key[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int count = 0;                  // 0: this geometry uses the regular grid
        int n_seams = 0;
        int max_rows = 0;               // the tallest item
        srcnn::host::DevBuf dev, dev_seams;
        srcnn::host::DevBuf dev_winmap;              // [n_strips][rows] bytes: 1 = the row lies in a seam window of that strip (separated plans)
        bool separated = false;         // seam windows of neighbouring strips share no row: one seam launch (plan_items_balanced())
        unsigned long stamp = 0;        // last use, for eviction
    };
    static constexpr int kItemTables = 32;
    ItemTable item_tables[kItemTables];
    unsigned long item_clock = 0;
    int last_launch[7] = {0, 0, 0, 0, 0, 0, 0};      // tuning build: geometry_report() of the last strip launch, and its frames
    // host copy of the uploaded tables in convdata.h order: the per-call weight arguments of the reference surface
    // (srcnn_conv99x11 / srcnn_conv55) are compared against it, and equal tables are not packed or uploaded again
    std::vector<float> host_raw = std::vector<float>(8129, 0.f);
    // pinned staging of the reference surface's 32 planes (two slots, alternating) and of single planes
    void *pin_plane[2] = {nullptr, nullptr};
    size_t pin_plane_cap = 0;
    // row-striped multi-device step (srcnn_forward_y_striped*): second stream for the halo copies, band inputs
    // [6 halo rows | 12 own rows] / [12 own rows | 6 halo rows], events ordering the two streams
    hipStream_t halo_stream = nullptr;
    hipEvent_t halo_ready = nullptr, bands_done = nullptr;
    bool bands_pending = false;
    srcnn::host::DevBuf band_top, band_bot, stripe_ext;
    // ... one-launch form (float32 MFMA kernel, StripParams::src_top).  With peer access (or neighbours on the same device) the
    // kernel reads the neighbours' edge rows WHERE THEY LIE, over xGMI: no copy, no event.  Only when a link refuses peer
    // access are the 6 halo rows either side copied (staged by the runtime) into buffers of their own, kHaloSets sets used in
    // turn, so that the copies of a step run while the kernels of the steps before it still read the other sets;
    // halo_free[i] = the launch that last read set i has finished
    static constexpr int kHaloSets = 4;
    srcnn::host::DevBuf halo_top[kHaloSets], halo_bot[kHaloSets];
    hipEvent_t halo_free[kHaloSets] = {nullptr, nullptr, nullptr, nullptr};
    bool halo_free_set[kHaloSets] = {false, false, false, false};
    unsigned long stripe_steps = 0;
    int halo_transport = 0;                // srcnn_halo_transport(): 0 none yet, 1 same device, 2 peer access (xGMI), 3 staged by the runtime
    std::vector<int> peer_state;           // per device id: 0 not asked yet, 2 peer access enabled, 3 refused
    // pipeline of a row-striped STREAM of planes (srcnn_forward_y_striped_frames): events behind the upload / the kernel / the
    // download of the plane in buffer b, and how many planes' events have been RECORDED so far -- a stream may only be told to
    // wait for an event another host thread has already recorded
    hipEvent_t sf_up[2] = {nullptr, nullptr}, sf_k[2] = {nullptr, nullptr}, sf_down[2] = {nullptr, nullptr};
    std::atomic<int> sf_gen_up{0}, sf_gen_k{0}, sf_abort{0};
    hipStream_t lane_stream[2] = {nullptr, nullptr};
    srcnn::host::DevBuf lane_in[2], lane_out[2];
    void *pin_in[2] = {nullptr, nullptr}, *pin_out[2] = {nullptr, nullptr};   // pinned host staging
    size_t pin_cap = 0;
    // Seam deferral (srcnn_set_seam_deferral): the seam launch of the last fused single-plane launch has NOT been queued yet; the
    // next such launch on the same stream carries its blocks (srcnn_strip_fold_kernel), anything else on the context queues it
    // first (flush_seams(): every entry point through BIND, the item-table eviction, srcnn_flush, srcnn_destroy).
    bool defer_seams = false;
    int defer_block = 0;                   // > 0: inside an entry point that uses the device launches itself and reads their output (no deferral)
    struct PendingSeams {
        bool valid = false;
        hipStream_t stream = nullptr;
        srcnn::FoldParams f{};
    } pending;
    float fix_delta = 0.f;                 // SRCNN_MODE_REFBYTES: flag threshold for the uploaded model (fixup_delta())
    float fix_margin = kFixMargin;         // ... the factor of its weight-proportional term (srcnn_set_fixup_margin)
    float fix_local = kFixLocal;           // ... the per-pixel threshold's factor per unit of the margin; 0 = the global threshold only (srcnn_set_fixup_local)
    float fix_local16 = kFixLocal16;       // ... and in SRCNN_MODE_REFBYTES16 (the split-f16 kernel's noise is a little wider)
    bool fix_strict = true;                // ... act on the monitor: a launch whose max_dev > delta / 2 is redone in the reference's arithmetic (fix_rerun_kernel)
    srcnn::host::DevBuf fix_totals;                     // ... and its counters accumulated over the context's launches (srcnn_fixup_stats)
    std::unique_ptr<srcnn::host::WorkerPool> pool;      // host threads of the several-GPUs calls this context leads (WorkerPool)
};

namespace srcnn {
namespace host {

int fail(srcnn_ctx *c, int code, const char *fmt, ...);

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail((ctx), e_ == hipErrorOutOfMemory ? SRCNN_ERR_NOMEM : SRCNN_ERR_HIP,     \
                        "%s failed: %s", #expr, hipGetErrorString(e_));                         \
    } while (0)

// Every entry point makes the context's device current for its own duration and puts the caller's device
// back on return (a framework sharing the thread keeps ITS current device).
struct DeviceScope {
    int prev = -1, rc = SRCNN_OK;
    explicit DeviceScope(srcnn_ctx *c)
    {
        if (!c) { rc = SRCNN_ERR_INVALID; return; }
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != c->device) {
            const hipError_t e = hipSetDevice(c->device);
            if (e != hipSuccess) {
                rc = fail(c, SRCNN_ERR_HIP, "hipSetDevice(%d) failed: %s", c->device, hipGetErrorString(e));
                prev = -1;
            }
        } else {
            prev = -1;      // nothing to restore
        }
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};
// While an entry point that calls the device launches ITSELF runs (host-buffer paths, the frame pipeline, the several-GPU calls:
// they read the launches' output right behind them), seam deferral is off: it is a contract with the DIRECT caller of a launch.
struct DeferBlock {
    srcnn_ctx *c;
    explicit DeferBlock(srcnn_ctx *ctx) : c(ctx) { ++c->defer_block; }
    ~DeferBlock() { --c->defer_block; }
    DeferBlock(const DeferBlock &) = delete;
    DeferBlock &operator=(const DeferBlock &) = delete;
};
// BIND_KEEP: the entry points whose launch can CARRY deferred seam work (run_strip decides); BIND: everything else queues it first.
#define BIND_KEEP(c)            \
    DeviceScope dev_scope_(c);  \
    if (dev_scope_.rc) return dev_scope_.rc
#define BIND(c)                                                        \
    BIND_KEEP(c);                                                      \
    if (int flush_rc_ = srcnn::host::flush_seams(c)) return flush_rc_; \
    srcnn::host::DeferBlock defer_block_(c)

int reserve(srcnn_ctx *c, DevBuf &b, size_t bytes);
void release(DevBuf &b);

constexpr int kHaloRows = 6;   // 4 input rows of the 9x9 layer + 2 feature rows of the 5x5 layer

// ---- srcnn_model.cpp ----
float fixup_delta(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, double margin = kFixMargin);
void pack_fragments(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, float *out);
void pack_fragments16(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, uint8_t *out);
void split16(float w, float scale, uint16_t *hi, uint16_t *lo);     // f16 bits of hi = f16(w scale), lo = f16(w scale - hi)
// SRCNN_MODE_BANDED16 (srcnn_spatial.cpp): the layer-1 bound for 8-bit input, the exponent that puts a bound in [2^14, 2^15),
// and W2 times its power-of-two scale as the split A-operand table of spatial_l2h_kernel (false: the model cannot be scaled)
double banded16_l1_bound(int C, const float *w1, const float *b1, double range = 255.0, int n1p = 64);
bool banded16_exponent(double bound, int *e);
bool banded16_pack_w2(int f2, const float *w2, uint16_t *table, int *e2, int n1p = 64, int n2p = 32);
bool split16_range_ok(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3);
int upload_weights(srcnn_ctx *c, const float *k99, const float *b99, const float *k11, const float *b11, const float *k55, float b55);
int use_layers12(srcnn_ctx *c, const float *kernel99, const float *bias99, const float *kernel11, const float *bias11);
int use_layer3(srcnn_ctx *c, const float *kernel, float bias);
inline bool has_model(const srcnn_ctx *c) { return c->has_l12 && c->has_l3; }
// The luma strip path may run: a 1-channel 9-1-5 model with replicate padding.  Every entry point that runs only that path (row
// stripes, halo buffers, several GPUs, unfused, per-layer device calls, the row bands of srcnn_forward_y) tests this one
// predicate; srcnn_forward_y_dev sends the other 1-channel models to the banded path and refuses a colour model.
// SRCNN_MODE_BANDED16 runs every model on the banded path, so none of these entry points runs in it -- but for the per-filter
// calls on host planes (srcnn_conv99x11, srcnn_conv55: per_filter is set while they run), which ignore every mode.
// A wide model (srcnn_set_model_shape with more than 64 / 32 filters) runs on the banded path only.
inline bool wide_model(const srcnn_ctx *c) { return c->n1p > 64 || c->n2p > 32; }
inline bool luma_path_ok(const srcnn_ctx *c)
{
    return c->channels == 1 && c->f2 == 1 && !wide_model(c) && c->padding != SRCNN_PAD_ZERO &&
           (c->mode != SRCNN_MODE_BANDED16 || c->per_filter);
}
void drop_spatial_model(srcnn_ctx *c);

// the entry points that run the 9-1-5 path with replicate padding only (row stripes, halo buffers, several GPUs, unfused,
// per-layer device calls; under SRCNN_PAD_ZERO also the per-filter calls): the message names the model, the padding or, in
// SRCNN_MODE_BANDED16, the mode (banded_entry: `what` does run the banded path, so the mode is not what blocks it)
int refuse_spatial(srcnn_ctx *c, const char *what, bool banded_entry = false);
// ---- srcnn_spatial.cpp: the banded path (layer 1 -> spatial layer 2 -> layer 3 per row band) ----
// n_frames planes of the loaded model (c->channels, c->f2, c->padding; refused with SRCNN_ERR_STATE where the mode, the padding
// or the way the model was loaded has no banded arithmetic): input byte c of pixel (y, x) at src[y * src_stride + x * px_step +
// c * ch_step] (1 channel: px_step 1, ch_step 0), output (and pre, at the same element offsets) pixels of c->channels bytes.
// The planes of one call: u8 (f32 false: src / dst point at bytes, strides in bytes, pre optional) or float32 (the float image
// path: strides in floats, channel o of the output at dst + o * dst_ch_pitch, px_step 1, no pre).
struct BandedPlanes {
    bool f32 = false;
    const void *src = nullptr;
    size_t src_stride = 0, ch_step = 0, src_frame_pitch = 0;
    int px_step = 1;
    void *dst = nullptr;
    size_t dst_stride = 0, dst_ch_pitch = 0, dst_frame_pitch = 0;
    float *pre = nullptr;
    // A row stripe (srcnn_model_rows*_dev, srcnn_model_color_rows*_dev, srcnn_model_rows*_f32_dev; one frame): output rows
    // [row_begin, row_end) of the width x height image.  src starts at image row src_row0, dst and pre at image row dst_row0.  With
    // halo_top / halo_bot the R = 6 + (f2 - 1) / 2 rows above src_row0 / from src_row0 + src_rows on come from those buffers (row
    // stride halo_stride, and for float planes channel pitch halo_ch_pitch, in elements as src_stride); null: src holds them.
    bool rows = false;
    int row_begin = 0, row_end = 0, src_row0 = 0, src_rows = 0, dst_row0 = 0;
    const void *halo_top = nullptr, *halo_bot = nullptr;
    size_t halo_stride = 0, halo_ch_pitch = 0;
};
int forward_banded(srcnn_ctx *c, const BandedPlanes &io, int width, int height, int n_frames);
int forward_banded(srcnn_ctx *c, const uint8_t *src, size_t src_stride, int px_step, size_t ch_step, size_t src_frame_pitch,
                   uint8_t *dst, size_t dst_stride, size_t dst_frame_pitch, int width, int height, int n_frames, float *pre);
// the gate of the stripe entry points: SRCNN_OK, or SRCNN_ERR_STATE and the reason.  kind: what the entry point takes
enum StripeKind { STRIPE_Y = 0, STRIPE_COLOR = 1, STRIPE_F32 = 2 };    // one byte channel, 3-byte pixels, 1 or 3 float planes
int model_rows_refusal(srcnn_ctx *c, StripeKind kind = STRIPE_Y);
// the float planes of a call (C channels x n_frames frames): elements spanned from the first, and whether the planes the call
// WRITES are disjoint; the gate of srcnn_forward_f32 for srcnn_process_f32*
size_t f32_span(int C, size_t stride, size_t ch_pitch, size_t frame_pitch, int width, int height, int n_frames);
bool f32_planes_disjoint(int C, size_t stride, size_t ch_pitch, size_t frame_pitch, int width, int height, int n_frames);
int forward_f32_refusal(srcnn_ctx *c);
constexpr size_t kSpatialWorkBytes = (size_t)512 << 20;     // bound of the two band maps (include/srcnn_amd.h, srcnn_set_model)
extern const char *const kNoModel;

// ---- srcnn_plan.cpp ----
struct Plan {
    int seg_rows, n_strips, n_segs;
};
Plan make_plan(const srcnn_ctx *c, int width, int rows, int n_frames, int halo, int wgs_per_cu = 2, int col_halo = -1);
// Explicit work items for a launch that fits the GPU in ONE round with two workgroups per CU.
// The hardware hands the first n_cu blocks wave slot 0 of every CU; the MFMA pipe is arbitrated by
// age, so those run faster than the block that joins them later (tools/diag_stamps.py).  Exactly
// 2*n_cu items are made: every strip is cut into k or k+1 segments, the "fast" ones (first n_cu
// blocks) (1+skew) tall, the "slow" ones (1-skew) tall, so that all slots are used and the two
// workgroups of a CU finish together.  Placement only affects speed; the items tile the rows exactly.
// With ONE workgroup per CU (the pipelined split-f16 kernel) there are n_cu items of plain equal height
// per strip.  With `want_seams` the boundaries between the items of a strip become seams
// (srcnn_kernels.h): the items carry the ids of the seams above / below them, `seams` lists
// {strip, boundary row} per id.  `items` holds ITEM_INTS ints per block in block order; empty when the
// geometry does not qualify (the regular grid is used instead).
struct ItemPlan {
    std::vector<int> items, seams;
    bool separated = false;        // no two seams of neighbouring strips closer than SEAM_ROWS rows (plan_items_balanced())
    int count() const { return (int)items.size() / ITEM_INTS; }
    int n_seams() const { return (int)seams.size() / 2; }
};
ItemPlan plan_items(int n_cu, int n_strips, int row_begin, int row_end, int skew_pct, int wgs_per_cu = 2, bool want_seams = false,
                    int extra_top = 0, int extra_bot = 0);
constexpr int kSkewPercent = 10;       // how much taller / shorter than the mean the first- / later-dispatched item of a CU is made
// report: null for a launch (the context's cache, device tables uploaded); else nothing on the device is touched and the
// cache stays as it is -- a cached table is returned as found, any other geometry is planned into *report (host fields only)
int build_items(srcnn_ctx *c, int n_strips, int row_begin, int row_end, int height, int wgs_per_cu, bool want_seams,
                const srcnn_ctx::ItemTable **table, srcnn_ctx::ItemTable *report = nullptr);
// The geometry of ONE strip launch, decided in one place (strip_geometry) for run_strip(), which launches from it, and for
// srcnn_query_plan(), which reports from it.
struct StripGeometry {
    bool split16 = false, fused32 = false;          // the fused pass on the split-f16 / the float32 kernel
    int tune = 0;                                   // the honoured bits of SRCNN_DEBUG_TUNE
    Plan grid{0, 0, 0};                             // the regular grid: segment rows, strips, segments (items == 0)
    int strips_total = 0;                           // strips of the plane
    const srcnn_ctx::ItemTable *table = nullptr;    // the item plan asked for, if any: count, seams, separated, tallest item
    int items = 0;                                  // explicit work items per frame (table->count); 0: the regular grid
    int items_per_cu = 0;                           // ... and how many of them share a compute unit
    bool col_seams = false;                         // strips of FW columns: the launch exports column seams
};
// mode: MODE_FUSED / MODE_L12 / MODE_L3; rows [row_begin, row_end) of a width x height plane, n_frames in the launch.
// report: as build_items() -- null for a launch, else a table to plan into without touching the device or the cache.
int strip_geometry(srcnn_ctx *c, int mode, int width, int height, int row_begin, int row_end, int n_frames, StripGeometry *g,
                   srcnn_ctx::ItemTable *report = nullptr);
// the six numbers of srcnn_query_plan for `frames` frames launched with this geometry
void geometry_report(const StripGeometry &g, int mode, int frames, int out[6]);
int split16_wgs_per_cu(bool split16);
int seam_scratch_for_stream(srcnn_ctx *c, srcnn_ctx::SeamScratch **out);
bool cseam_pays(int width);
constexpr int kItemBatchMax = 32, kItemBatchChunk = 8, kGridBatchChunk = 64;
bool f32_mfma(const srcnn_ctx *c);
int frames_per_launch(const srcnn_ctx *c, int width, int height, int n_frames);

// ---- srcnn_launch.cpp ----
bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes);
size_t span_elems(size_t stride, size_t frame_pitch, int width, int height, int n_frames);
bool bad_plane(const void *p, size_t stride, int w, int h);
bool bad_pitch(size_t plane_pitch);
// may_defer: the caller is one of the device entry points whose contract allows seam deferral (srcnn_set_seam_deferral)
int run_strip(srcnn_ctx *c, int mode, StripParams p, int n_frames, int fix_frame = 0, int fix_frames = 1, bool may_defer = false);
int flush_seams(srcnn_ctx *c);

// ---- srcnn_resize_f32.cpp: the float32 cubic resize ----
// the one table builder (also srcnn_cubic_f32_taps), and the tables of a geometry on the device
void cubic_f32_taps(int n_src, int n_dst, int *first, float *coef);
struct ResizeTablesF32 {
    const int *xfirst, *yfirst;
    const float *xcoef, *ycoef;
};
int ensure_tables_f32(srcnn_ctx *c, int sw, int sh, int dw, int dh, ResizeTablesF32 *t);
// the antialiased table of one axis (also srcnn_cubic_aa_f32_taps, where include/srcnn_amd.h writes its float64 operations out):
// the largest count of the axis; coef null: that and nothing else; else first[d], count[d], coef[d * max_taps + j] (zero beyond
// count[d]), SRCNN_ERR_INVALID for max_taps below the largest count.  (The device tables and the launch: srcnn_image.h.)
int cubic_aa_f32_taps(int n_src, int n_dst, int *first, int *count, float *coef, int max_taps);
// Pillow's table of one axis for uint8 pictures (also srcnn_pil_taps): the same conventions, int32 coefficients with 22
// fractional bits; filter: SRCNN_PIL_BILINEAR or SRCNN_PIL_BICUBIC (checked by the caller)
int pil_taps(int n_src, int n_dst, int filter, int *first, int *count, int32_t *coef, int max_taps);

// ---- srcnn_host.cpp ----
void cubic_table(int n_src, int n_dst, int *ofs, short *coef);
int ensure_lanes(srcnn_ctx *c, size_t bytes);      // the two lane streams, lane_in / lane_out device buffers and pinned staging of >= bytes

// rows of `width` elements between a packed buffer and a strided one, split over a few threads
template <typename T>
void copy_rows_mt(T *dst, size_t dst_stride, const T *src, size_t src_stride, int width, int height)
{
    static const int n_thr = [] {
        const char *e = SRCNN_DEBUG_ENV("SRCNN_HOST_COPY_THREADS");
        const int hw = (int)std::thread::hardware_concurrency();
        return std::max(1, e ? std::atoi(e) : std::min(8, hw > 0 ? hw / 2 : 4));
    }();
    auto part = [=](int y0, int y1) {
        if (dst_stride == (size_t)width && src_stride == (size_t)width)
            std::memcpy(dst + (size_t)y0 * width, src + (size_t)y0 * width, (size_t)(y1 - y0) * width * sizeof(T));
        else
            for (int y = y0; y < y1; ++y) std::memcpy(dst + (size_t)y * dst_stride, src + (size_t)y * src_stride, (size_t)width * sizeof(T));
    };
    const int nt = (int)std::min<size_t>((size_t)n_thr, std::max<size_t>(1, (size_t)width * height * sizeof(T) >> 20));   // >= 1 MB per thread
    if (nt <= 1) { part(0, height); return; }
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(part, (int)((long)height * t / nt), (int)((long)height * (t + 1) / nt));
    part(0, height / nt);
    for (auto &th : pool) th.join();
}

}  // namespace host
}  // namespace srcnn
