// Stand-alone driver for csrc/resample_coeffs.h under -fsanitize=address,undefined (tests/test_image_front_host.py): the two
// phases as the library runs them -- query ksize, fill -- into heap buffers of exactly the stated sizes, so that any write past
// a table or the scratch row is an AddressSanitizer report; then the invariants the kernels rely on.
#include <stdio.h>

#include <vector>

#include "../../sculptmate_amd/csrc/resample_coeffs.h"

static int check_pair(int in_size, int out_size) {
    const int ksize = sculpt::resample_lanczos_ksize(in_size, out_size);
    if (ksize < 7) return printf("%d -> %d: ksize %d\n", in_size, out_size, ksize), 1;
    std::vector<int32_t> bounds((size_t)out_size * 2), kk((size_t)out_size * ksize);
    std::vector<double> scratch((size_t)ksize);
    if (sculpt::resample_lanczos_fill(in_size, out_size, ksize, bounds.data(), kk.data(), scratch.data()))
        return printf("%d -> %d: fill failed\n", in_size, out_size), 1;
    if (!sculpt::resample_lanczos_fill(in_size, out_size, ksize + 2, bounds.data(), kk.data(), scratch.data()))
        return printf("%d -> %d: a wrong ksize was accepted\n", in_size, out_size), 1;
    for (int xx = 0; xx < out_size; ++xx) {
        const int lo = bounds[2 * xx], n = bounds[2 * xx + 1];
        if (lo < 0 || n < 1 || n > ksize || lo + n > in_size) return printf("%d -> %d: window [%d, +%d) at %d\n", in_size, out_size, lo, n, xx), 1;
        long sum = 0;
        for (int x = 0; x < ksize; ++x) {
            if (x >= n && kk[(size_t)xx * ksize + x] != 0) return printf("%d -> %d: weight past the window at %d\n", in_size, out_size, xx), 1;
            sum += kk[(size_t)xx * ksize + x];
        }
        // the weights sum to one in 2^-22 units up to one rounding per tap
        if (sum < (1L << 22) - ksize || sum > (1L << 22) + ksize) return printf("%d -> %d: weights sum to %ld at %d\n", in_size, out_size, sum, xx), 1;
    }
    return 0;
}

int main() {
    const int pairs[][2] = {{53, 320}, {700, 320}, {320, 701}, {320, 97}, {1500, 1024}, {7, 2}, {5, 3}, {1, 4}, {64, 64}, {1, 1},
                            {4096, 320}, {3072, 320}, {320, 4096}, {32768, 1}, {1, 32768}};
    for (const auto &p : pairs)
        if (check_pair(p[0], p[1])) return 1;
    if (sculpt::resample_lanczos_ksize(0, 4) || sculpt::resample_lanczos_ksize(4, 0) || sculpt::resample_lanczos_ksize(1 << 20, 4)) {
        printf("a size out of range was accepted\n");
        return 1;
    }
    printf("asan_resample_coeffs ok\n");
    return 0;
}
