// Pillow's 8-bit LANCZOS resample, the coefficient side: plain host C++ (libm sin, double arithmetic), no HIP, so that it can be
// compiled alone (tests/native/asan_resample_coeffs.cpp) and called without a GPU (sculpt_resample_lanczos_*).
//
// Restated from the published behaviour of Image.resize(size, LANCZOS) on 8-bit images: for inSize -> outSize
//   scale = inSize / outSize, fs = max(scale, 1), support = 3 fs, ksize = (int)ceil(support) * 2 + 1
// and per output index xx
//   center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0), n = min((int)(center + support + 0.5), inSize) - xmin
//   w[x] = lanczos((x + xmin - center + 0.5) * (1 / fs)) for x < n, summed in index order into ww, each divided by ww when ww != 0
//   k[x] = (int)(w * 2^22 + 0.5) for w >= 0, (int)(w * 2^22 - 0.5) for w < 0; k[x] = 0 for n <= x < ksize.
// Every operation is an IEEE double operation in this order: the table is the library's to the bit as long as sin() is the same
// libm function, which is why it is computed here and not on the device.
#pragma once
#include <math.h>
#include <stdint.h>

namespace sculpt {

static constexpr int RESAMPLE_PRECISION_BITS = 32 - 8 - 2;
static constexpr int RESAMPLE_MAX_SIZE = 1 << 15;   // image sides this path accepts (a grid row per image row; tables far below 2^31 entries)

static inline double resample_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;
    return sin(x) / x;
}

static inline double resample_lanczos(double x) {
    if (-3.0 <= x && x < 3.0) return resample_sinc(x) * resample_sinc(x / 3);
    return 0.0;
}

// taps per output index, or 0 when the sizes are outside [1, RESAMPLE_MAX_SIZE]
static inline int resample_lanczos_ksize(int in_size, int out_size) {
    if (in_size < 1 || out_size < 1 || in_size > RESAMPLE_MAX_SIZE || out_size > RESAMPLE_MAX_SIZE) return 0;
    double fs = (double)in_size / out_size;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(3.0 * fs) * 2 + 1;
}

// bounds[2 xx] = xmin, bounds[2 xx + 1] = n (taps used: xmin + n <= in_size, n <= ksize); kk[xx * ksize + x] as above.
// `scratch` holds ksize doubles.  Returns 0, or 1 when ksize is not resample_lanczos_ksize(in_size, out_size).
static inline int resample_lanczos_fill(int in_size, int out_size, int ksize, int32_t *bounds, int32_t *kk, double *scratch) {
    if (ksize < 1 || ksize != resample_lanczos_ksize(in_size, out_size)) return 1;
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * fs, ss = 1.0 / fs;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        int n = xmax - xmin;
        if (n < 0) n = 0;            // (cannot happen for sizes >= 1; the tables' consumers rely on 0 <= n <= ksize)
        if (n > ksize) n = ksize;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            const double w = resample_lanczos((x + xmin - center + 0.5) * ss);
            scratch[x] = w;
            ww += w;
        }
        int32_t *k = kk + (size_t)xx * ksize;
        for (int x = 0; x < n; ++x) {
            const double w = ww != 0.0 ? scratch[x] / ww : scratch[x];
            k[x] = w < 0 ? (int32_t)(-0.5 + w * (1 << RESAMPLE_PRECISION_BITS)) : (int32_t)(0.5 + w * (1 << RESAMPLE_PRECISION_BITS));
        }
        for (int x = n; x < ksize; ++x) k[x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
    }
    return 0;
}

}  // namespace sculpt
