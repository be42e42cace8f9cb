// san_pil_taps.cpp -- sanitizer harness for srcnn_pil_taps, the host-only table builder of Pillow's resize
// (srcnn_cpp_amd/csrc/srcnn_resize_f32.cpp).  tests/test_pil_cpu.py compiles that file itself with the host compiler and
// -fsanitize=address,undefined (no device code; -ffunction-sections and --gc-sections drop the entry points this harness never
// reaches, so nothing else of the library is linked), and runs this on the CPU.  No HIP call is made: nothing here needs a device.
// Every table is written into buffers of exactly the size the sizing call asks for: one int beyond them is a sanitizer error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" int srcnn_pil_taps(int src_n, int dst_n, int filter, int *first, int *count, int32_t *coef, int max_taps);

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "CHECK failed: %s (line %d; %d -> %d, filter %d)\n", #cond, __LINE__, s, n, f); return 1; } \
    } while (0)

int main()
{
    std::vector<int> sizes;
    for (int v = 1; v <= 70; ++v) sizes.push_back(v);
    for (int v : {97, 127, 128, 129, 200, 255, 256, 257, 1080, 1920, 2160, 3840, 8191}) sizes.push_back(v);
    long tables = 0, worst_sum = 0;
    for (int f : {2, 3})
        for (int s : sizes)
            for (int n : sizes) {
                if ((long)s * n > 3840L * 3840) continue;
                const int k = srcnn_pil_taps(s, n, f, nullptr, nullptr, nullptr, 0);
                CHECK(k > 0 && k <= s);
                std::vector<int> first((size_t)n), count((size_t)n);
                std::vector<int32_t> coef((size_t)n * k);
                CHECK(srcnn_pil_taps(s, n, f, first.data(), count.data(), coef.data(), k) == k);
                int kmax = 0;
                for (int d = 0; d < n; ++d) {
                    CHECK(first[d] >= 0 && count[d] > 0 && count[d] <= k && first[d] + count[d] <= s);
                    CHECK(d == 0 || (first[d] >= first[d - 1] && first[d] + count[d] >= first[d - 1] + count[d - 1]));
                    kmax = count[d] > kmax ? count[d] : kmax;
                    long sum = 0, sum_abs = 0;
                    for (int j = 0; j < k; ++j) {
                        const long c = coef[(size_t)d * k + j];
                        CHECK(j < count[d] || c == 0);
                        sum += c;
                        sum_abs += c < 0 ? -c : c;
                    }
                    // the weights were normalised to 1: the integers add up to 2^22 within half a unit per tap; the int32 bound
                    CHECK(sum >= (1L << 22) - k && sum <= (1L << 22) + k);
                    CHECK(sum_abs < (1L << 23));
                    worst_sum = sum_abs > worst_sum ? sum_abs : worst_sum;
                }
                CHECK(kmax == k);
                ++tables;
            }
    {   // the refusals
        int s = 5, n = 7, f = 3, one = 0;
        int32_t c = 0;
        CHECK(srcnn_pil_taps(0, n, f, nullptr, nullptr, nullptr, 0) < 0 && srcnn_pil_taps(s, -1, f, nullptr, nullptr, nullptr, 0) < 0);
        CHECK(srcnn_pil_taps(s, n, 1, nullptr, nullptr, nullptr, 0) < 0 && srcnn_pil_taps(s, n, 4, nullptr, nullptr, nullptr, 0) < 0);
        CHECK(srcnn_pil_taps(s, n, f, nullptr, &one, &c, 8) < 0 && srcnn_pil_taps(s, n, f, &one, nullptr, &c, 8) < 0);
        std::vector<int> first((size_t)n), count((size_t)n);
        std::vector<int32_t> coef((size_t)n * 3);
        CHECK(srcnn_pil_taps(s, n, f, first.data(), count.data(), coef.data(), 3) < 0);      // 4 taps needed
    }
    std::printf("ok: %ld tables, largest sum |c| %ld (%.4f x 2^22)\n", tables, worst_sum, (double)worst_sum / (double)(1 << 22));
    return 0;
}
