// srcnn_cli.cpp -- command-line front end with the reference tool's interface
// (reference: parseArgs / printTitle / printHelp /
// pthreadcall / main, src/srcnn.cpp:331-731), running the pipeline on the GPU.
//
//   srcnn_amd [--scale=F] [--noverbose] [--help] [--weights=FILE] [--padding=zero|replicate] [--timing] [--refbytes]
//             source [output]
//
// Same argument rules as the reference: --scale= must be > 0 (default 2.0,
// src/srcnn.cpp:40,359-370); first free argument = source, second = output;
// default output "<name>_resized<ext>" (:396-416); without a source the title
// and help are printed and the exit code is 0 (:709-715).  Exit codes: -1 image
// load failure or scale too small (:479,:493), -10 no output (:684), 0 success.
// The timed region ("Performace : N ms took.", :505,:659,:690) covers colour
// conversion, resize, the conv path and the conversion back, as in the reference
// -- here including the PCIe transfers and, since it is the context's first call,
// the kernels' first launch and the buffer allocations -- and excludes file decode/encode.
// Differences: image codecs are own PNG/PPM code (tools/image_io.hpp), not
// OpenCV's, so JPEG etc. are not read; the model is loaded from a weight file
// (--weights=, $SRCNN_WEIGHTS, or data/ next to libsrcnn_amd.so) instead
// of being compiled in from convdata.h.
// --timing prints where the PROCESS's time goes, from the first instruction of main() to the written file (the reference's only
// use case is one image per process, src/srcnn.cpp:707-731): file decode, HIP runtime start, srcnn_create (stream + interlock
// probe, which loads the code object), weights, the timed region (the context's FIRST call), file encode.  tests/checks/time_cli.py adds what
// lies in front of main() (exec, dynamic linking) from the outside.  --refbytes selects SRCNN_MODE_REFBYTES (the reference's
// bytes); the default is the float32 MFMA mode.
#include <dlfcn.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "image_io.hpp"
#include "srcnn_amd.h"

namespace {

struct Options {
    float scale = 2.0f;
    bool verbose = true, help = false, copy = false, timing = false, refbytes = false;
    int padding = SRCNN_PAD_REPLICATE;
    std::string me, src, dst, weights, error;
};

bool starts_with(const std::string &s, const char *p) { return s.rfind(p, 0) == 0; }

bool parse(int argc, char **argv, Options &o)
{
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        if (i == 0) {
            const size_t cut = a.find_last_of("/\\");
            o.me = cut == std::string::npos ? a : a.substr(cut + 1);
        } else if (starts_with(a, "--scale=")) {
            const float v = (float)std::atof(a.c_str() + 8);
            if (v > 0.f) o.scale = v;
        } else if (starts_with(a, "--noverbose")) {
            o.verbose = false;
        } else if (starts_with(a, "--help")) {
            o.help = true;
        } else if (a == "--copy") {          // codec self-test: decode source, encode output, no GPU
            o.copy = true;
        } else if (a == "--timing") {
            o.timing = true;
        } else if (a == "--refbytes") {
            o.refbytes = true;
        } else if (starts_with(a, "--weights=")) {
            o.weights = a.substr(10);
        } else if (starts_with(a, "--padding=")) {
            const std::string v = a.substr(10);
            if (v == "zero") o.padding = SRCNN_PAD_ZERO;
            else if (v == "replicate") o.padding = SRCNN_PAD_REPLICATE;
            else o.error = "--padding=" + v + " : expected zero or replicate";
        } else if (o.src.empty()) {
            o.src = a;
        } else if (o.dst.empty()) {
            o.dst = a;
        }
    }
    if (o.help || o.src.empty()) return false;
    if (o.dst.empty()) {
        const size_t dot = o.src.find_last_of('.');
        o.dst = dot == std::string::npos ? o.src + "_resized"
                                         : o.src.substr(0, dot) + "_resized" + o.src.substr(dot);
    }
    return true;
}

void title(const Options &o)
{
    std::printf("%s : Super-Resolution with deep Convolutional Neural Networks\n", o.me.c_str());
    std::printf("MI355X (gfx950) HIP path, C ABI version %d; interface of SRCNN_Cpp's srcnn tool\n",
                srcnn_abi_version());
}

void help(const Options &o)
{
    std::printf("\n    usage : %s (options) [source file name] ([output file name])\n\n", o.me.c_str());
    std::printf("    _options_:\n\n");
    std::printf("        --scale=( ratio: 0.1 to .. ) : scaling by ratio.\n");
    std::printf("        --noverbose                  : turns off all verbose\n");
    std::printf("        --weights=FILE               : model blob, b1|W1|b2|W2|b3|W3: 8129 (9-1-5), 24513 (9-3-5) or 57281 (9-5-5) floats\n");
    std::printf("                                       colour (BGR channels): 20099, 36483 or 69251 floats\n");
    std::printf("        --padding=zero|replicate     : padding of every layer's input (default replicate; zero = PyTorch's nn.Conv2d)\n");
    std::printf("        --help                       : this help\n\n");
}

bool load_weights(const Options &o, const char *argv0, std::vector<float> &blob)
{
    std::vector<std::string> cand;
    if (!o.weights.empty()) cand.push_back(o.weights);
    if (const char *e = std::getenv("SRCNN_WEIGHTS")) cand.push_back(e);
    std::string dir = argv0;
    const size_t cut = dir.find_last_of('/');
    dir = cut == std::string::npos ? "." : dir.substr(0, cut);
    Dl_info info;                                  // the blob shipped next to libsrcnn_amd.so
    if (dladdr(reinterpret_cast<void *>(&srcnn_create), &info) && info.dli_fname) {
        std::string lib = info.dli_fname;
        const size_t lc = lib.find_last_of('/');
        cand.push_back((lc == std::string::npos ? std::string(".") : lib.substr(0, lc)) + "/data/srcnn915_weights.f32");
    }
    cand.push_back(dir + "/../srcnn_cpp_amd/data/srcnn915_weights.f32");
    cand.push_back(dir + "/srcnn915_weights.f32");
    cand.push_back("srcnn_cpp_amd/data/srcnn915_weights.f32");
    // a 9-1-5, 9-3-5 or 9-5-5 blob (include/srcnn_amd.h, srcnn_set_model): 8,129 / 24,513 / 57,281 floats, or a colour one
    // (srcnn_set_model_color, channels in BGR order): 20,099 / 36,483 / 69,251 floats; a file of any other size named by
    // --weights=, or one that cannot be opened, is an error, not a reason to fall back on the shipped model: the candidate that
    // --weights= names (the first, where the option is given) ends the search whatever becomes of it
    for (size_t i = 0; i < cand.size(); ++i) {
        const bool named = i == 0 && !o.weights.empty();
        FILE *f = std::fopen(cand[i].c_str(), "rb");
        if (!f) {
            if (named) return false;
            continue;
        }
        std::vector<float> buf(69251 + 1);
        const size_t n = std::fread(buf.data(), 4, buf.size(), f);
        std::fclose(f);
        if (n == 8129 || n == 24513 || n == 57281 || n == 20099 || n == 36483 || n == 69251) {
            buf.resize(n);
            blob.swap(buf);
            return true;
        }
        if (named) return false;
    }
    return false;
}

}  // namespace

// --timing: milliseconds since main() began, one line per phase
struct Phases {
    using clock = std::chrono::steady_clock;
    clock::time_point t0 = clock::now(), last = t0;
    bool on = false;
    void mark(const char *what)
    {
        const auto now = clock::now();
        if (on) std::printf("- timing : %-44s %9.3f ms   (at %9.3f)\n", what, std::chrono::duration<double, std::milli>(now - last).count(),
                            std::chrono::duration<double, std::milli>(now - t0).count());
        last = now;
    }
};

// the HIP runtime's own start, separated from srcnn_create for --timing: hipInit + hipGetDeviceCount through the runtime the
// library is linked against (already mapped: RTLD_NOLOAD finds it; the tool itself links no HIP)
void start_hip_runtime()
{
    void *h = dlopen("libamdhip64.so", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("libamdhip64.so.7", RTLD_NOW | RTLD_NOLOAD);
    if (!h) return;
    using init_fn = int (*)(unsigned);
    using count_fn = int (*)(int *);
    if (auto f = reinterpret_cast<init_fn>(dlsym(h, "hipInit"))) (void)f(0);
    int n = 0;
    if (auto f = reinterpret_cast<count_fn>(dlsym(h, "hipGetDeviceCount"))) (void)f(&n);
}

int main(int argc, char **argv)
{
    Phases ph;
    Options o;
    if (!parse(argc, argv, o)) {
        title(o);
        help(o);
        std::fflush(stdout);
        return 0;
    }
    if (o.error.empty() && o.padding == SRCNN_PAD_ZERO && o.refbytes)
        o.error = "--padding=zero and --refbytes : the reference's bytes are those of replicate padding";
    if (!o.error.empty()) {
        std::printf("- argument error : %s\n", o.error.c_str());
        return -1;
    }
    if (o.verbose) {
        title(o);
        std::printf("\n- Scale multiply ratio : %.2f\n", o.scale);
    }
    ph.on = o.timing;
    imgio::Image in = imgio::imread(o.src);
    ph.mark("decode the source file");
    if (in.empty()) {
        if (o.verbose) std::printf("- load failure : %s\n", o.src.c_str());
        return -1;
    }
    if (o.verbose) std::printf("- Image load : %s\n", o.src.c_str());
    if (o.copy) return imgio::imwrite(o.dst, in.bgr.data(), in.width, in.height) ? 0 : -10;
    int ow = 0, oh = 0;
    if (srcnn_scaled_size(in.width, in.height, o.scale, &ow, &oh) != SRCNN_OK) {
        if (o.verbose) std::printf("- Image scale error : ratio too small.\n");
        return -1;
    }
    std::vector<float> w;
    if (!load_weights(o, argv[0], w)) {
        std::printf("- model load failure (use --weights=FILE or $SRCNN_WEIGHTS)\n");
        return -1;
    }
    ph.mark("load the model file");
    if (o.timing) {
        start_hip_runtime();
        ph.mark("HIP runtime start (hipInit, device count)");
    }
    srcnn_ctx *ctx = nullptr;
    int rc = srcnn_create(&ctx, 0);
    ph.mark("srcnn_create (stream, interlock probe)");
    if (rc != SRCNN_OK) {
        std::printf("- GPU failure : no usable gfx950 device (error %d); there is no CPU fallback\n", rc);
        return -1;
    }
    const bool color = w.size() == 20099 || w.size() == 36483 || w.size() == 69251;
    const int f2 = (w.size() == 8129 || w.size() == 20099) ? 1 : ((w.size() == 24513 || w.size() == 36483) ? 3 : 5);
    if (color) {        // b1 | W1 [64][3][9][9] | b2 | W2 | b3[3] | W3 [3][32][5][5]: process_bgr runs it on all three channels
        const float *b1 = w.data(), *w1 = b1 + 64, *b2 = w1 + 15552, *w2 = b2 + 32, *b3 = w2 + 2048 * f2 * f2, *w3 = b3 + 3;
        rc = srcnn_set_model_color(ctx, f2, w1, b1, w2, b2, w3, b3);
    } else {
        const float *b1 = w.data(), *w1 = b1 + 64, *b2 = w1 + 5184, *w2 = b2 + 32, *w3 = w2 + 2048 * f2 * f2 + 1;
        rc = f2 == 1 ? srcnn_set_weights(ctx, w1, b1, w2, b2, w3, w3[-1]) : srcnn_set_model(ctx, f2, w1, b1, w2, b2, w3, w3[-1]);
    }
    if (rc == SRCNN_OK && o.refbytes) rc = srcnn_set_mode(ctx, SRCNN_MODE_REFBYTES);
    if (rc == SRCNN_OK) rc = srcnn_set_padding(ctx, o.padding);
    ph.mark("srcnn_set_weights (pack + upload)");
    std::vector<unsigned char> out((size_t)ow * oh * 3);
    // (No warm-up call: the reference runs ONE picture per process, so the timed region below is the context's first call and
    // contains what a first call costs -- the first launch of every kernel, the staging buffers, the pinned host memory.  Round 4
    // ran a 16 x 16 picture first to keep that out of the "Performace" line: 10-15 ms of the process's wall clock for a smaller
    // number on a line nobody could reproduce with one invocation.)
    if (o.verbose) {
        std::printf("- Image converting to Y-Cr-Cb, resizing with bicubic interpolation,\n");
        std::printf("  convolutional layers I + II + III, converting to BGR (one GPU pipeline) : ");
        if (o.timing) std::printf("\n");
        std::fflush(stdout);
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (rc == SRCNN_OK)
        rc = srcnn_process_bgr(ctx, in.bgr.data(), 3 * (size_t)in.width, in.width, in.height, o.scale, out.data(),
                               3 * (size_t)ow);
    const auto t1 = std::chrono::steady_clock::now();
    ph.mark("srcnn_process_bgr (the reference's timed region)");
    if (rc != SRCNN_OK) {
        if (o.verbose) std::printf("Failure.\n- %s\n", srcnn_last_error(ctx));
        srcnn_destroy(ctx);
        return -10;
    }
    if (o.verbose) {
        std::printf("Ok.\n- Writing result to %s : ", o.dst.c_str());
        if (o.timing) std::printf("\n");
        std::fflush(stdout);
    }
    const bool wrote = imgio::imwrite(o.dst, out.data(), ow, oh);
    ph.mark("encode + write the output file");
    if (o.verbose) std::printf(wrote ? "Ok.\n" : "Failure.\n");
    if (o.verbose)
        std::printf("- Performace : %u ms took.\n",
                    (unsigned)std::chrono::duration_cast<std::chrono::milliseconds>(t1 - t0).count());
    std::fflush(stdout);
    srcnn_destroy(ctx);
    ph.mark("srcnn_destroy");
    std::fflush(stdout);
    return wrote ? 0 : -10;
}
