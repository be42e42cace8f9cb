// process_srcnn_host.cpp -- a plain C++ host (no HIP headers) that calls srcnn::ProcessSRCNN (include/srcnn_amd.hpp), the
// buffer-level twin of the command-line tool's timed region, several times from ONE thread: every call after the first
// reuses the thread-local Session, at whatever geometry it is given.  tests/test_gpu_pipeline.py drives it.
//
//   process_srcnn_host weights.f32 OUT_PREFIX JOB...      JOB = FILE:W:H:SCALE, FILE raw B,G,R bytes or NULL (a null source)
//
// Before every call `out` holds five 0xAB bytes and the sizes 12345; a line per job says what the call returned and left:
//   job N rc=R w=W h=H size=S untouched=0|1
// and a call that returned 0 writes its bytes to OUT_PREFIX.N
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "srcnn_amd.hpp"

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: %s weights.f32 OUT_PREFIX FILE:W:H:SCALE...\n", argv[0]); return 2; }
    static float blob[8129];
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(blob, 4, 8129, f) != 8129) { std::fprintf(stderr, "bad weight file\n"); return 1; }
    std::fclose(f);
    // convdata.h order: b1[64] | W1[64][9][9] | b2[32] | W2[32][64] | b3 | W3[32][5][5]
    const float *b1 = blob;
    auto w1 = reinterpret_cast<const float(*)[9][9]>(blob + 64);
    const float *b2 = blob + 5248;
    auto w2 = reinterpret_cast<const float(*)[64]>(blob + 5280);
    const float b3 = blob[7328];
    auto w3 = reinterpret_cast<const float(*)[5][5]>(blob + 7329);

    const std::vector<unsigned char> sentinel(5, 0xAB);
    for (int j = 3; j < argc; ++j) {
        const std::string job = argv[j];
        const size_t npos = std::string::npos, c3 = job.rfind(':');
        const size_t c2 = c3 == npos || c3 == 0 ? npos : job.rfind(':', c3 - 1);
        const size_t c1 = c2 == npos || c2 == 0 ? npos : job.rfind(':', c2 - 1);
        if (c1 == npos) { std::fprintf(stderr, "bad job %s\n", argv[j]); return 2; }
        const std::string name = job.substr(0, c1);
        const unsigned w = (unsigned)std::atoi(job.substr(c1 + 1, c2 - c1 - 1).c_str());
        const unsigned h = (unsigned)std::atoi(job.substr(c2 + 1, c3 - c2 - 1).c_str());
        const float scale = (float)std::atof(job.substr(c3 + 1).c_str());
        std::vector<unsigned char> src;
        if (name != "NULL") {
            src.resize((size_t)w * h * 3);
            FILE *in = std::fopen(name.c_str(), "rb");
            if (!in || std::fread(src.data(), 1, src.size(), in) != src.size()) { std::fprintf(stderr, "bad source %s\n", name.c_str()); return 1; }
            std::fclose(in);
        }
        std::vector<unsigned char> out = sentinel;
        unsigned ow = 12345, oh = 12345;
        int rc;
        try {
            rc = srcnn::ProcessSRCNN(name == "NULL" ? nullptr : src.data(), w, h, scale, out, ow, oh, w1, b1, w2, b2, w3, b3);
        } catch (const srcnn::Error &e) {
            std::fprintf(stderr, "srcnn error %d: %s\n", e.code, e.what());
            return 3;
        }
        const int n = j - 3;
        std::printf("job %d rc=%d w=%u h=%u size=%zu untouched=%d\n", n, rc, ow, oh, out.size(),
                    (int)(out == sentinel && ow == 12345 && oh == 12345));
        if (rc == 0) {
            const std::string dst = std::string(argv[2]) + "." + std::to_string(n);
            FILE *o = std::fopen(dst.c_str(), "wb");
            if (!o || std::fwrite(out.data(), 1, out.size(), o) != out.size()) return 5;
            std::fclose(o);
        }
    }
    return 0;
}
