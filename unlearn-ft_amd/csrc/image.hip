// pdmk_image_prep / pdmk_image_prep_ex: the training transform of the image-caption loader (Resize(R, BILINEAR) ->
// CenterCrop / RandomCrop -> optional horizontal flip -> ToTensor -> Normalize(0.5, 0.5)) and CLIP's evaluation transform
// (Resize(R, BICUBIC) -> CenterCrop -> ToTensor -> Normalize(mean, std)) over a ragged batch of decoded 8-bit RGB images,
// bit-exact with Pillow's 8-bpc two-pass resample (libImaging/Resample.c, Pillow >= 7):
//   * per output coordinate: scale = in / out, filterscale = max(scale, 1), support = filterscale (triangle filter) or
//     2 * filterscale (cubic, a = -0.5), center = (xx + 0.5) * scale, taps [int(center - support + 0.5),
//     int(center + support + 0.5)) clipped to the input, w_i = filter((i + xmin - center + 0.5) * (1 / filterscale)),
//     normalised by their sequential double sum, then k_i = int(0.5 + w_i * 2^22) (int(-0.5 + w_i * 2^22) for w_i < 0);
//   * horizontal pass: (2^21 + sum_i px * k_i) >> 22, clipped to [0, 255] (uint8 intermediate; cubic sums can leave the
//     range on both sides); vertical pass likewise over the intermediate rows;
//   * x / 255 then (x - mean_c) / std_c in fp32 (divided, not multiplied by a reciprocal).
// Every double / float operation above is written out in the order Pillow / torch perform it; FP contraction is off for this
// file (an FMA would change the rounding of `center` or of the fixed-point coefficients, and with it the output bits).
//
// One workgroup per (output row band of BAND rows, image).  Only the crop window is computed: the band's output rows need
// source rows [ymin(first row), ymax(last row)); their horizontal pass (only the R columns of the crop) goes to LDS as uint8,
// in chunks of STAGE_BYTES when a large downscale needs more rows than fit, and each thread accumulates the vertical sums of
// its (row, column) outputs in registers across the chunks.  Source reads are aligned 4-byte loads; neighbouring threads
// read neighbouring words of the same row.  The vertical taps of one output row are held in LDS (KVMAX): the triangle filter
// needs at most 2 * ceil(in / out) + 1 of them, the cubic one 4 * ceil(in / out) + 1, so the largest downscale is 127x for
// bilinear and 63x for bicubic.
//
// pdmk_image_resize_u8 is the same bicubic resample with a rectangular window (the whole resized image, x and y scaled
// independently) and the bytes themselves as output: Pillow's Image.resize((W, H)).
// pdmk_resize_bilinear_u8 is NOT Pillow's resample but torch's CPU F.interpolate(mode="bilinear", align_corners=False) on the
// float image (two taps per axis whatever the scale, no antialiasing), the resize of clean-fid's legacy_pytorch FID mode; its
// source coordinate is the one explicit fma of this file.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int BAND = 4;                 // output rows per workgroup
constexpr int RMAX = 1024;              // largest output side
constexpr int KVMAX = 256;              // vertical taps per output row: downscale <= 127x bilinear, <= 63x bicubic
constexpr int STAGE_BYTES = 24 * 1024;  // horizontal-pass rows staged in LDS (uint8, [row][channel][column])
constexpr int PB = 22;                  // PRECISION_BITS

__device__ __forceinline__ double tri(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
// Pillow's bicubic_filter, a = -0.5, in its operation order
__device__ __forceinline__ double cubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Pillow's precompute_coeffs for one output coordinate xx: first tap, tap count, the filter centre and the weight sum
struct Axis {
    double scale, fs, support, ss;
};
template <bool CUBIC>
__device__ __forceinline__ Axis make_axis(int in, int out) {
    Axis a;
    a.scale = (double)in / (double)out;
    a.fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = (CUBIC ? 2.0 : 1.0) * a.fs;
    a.ss = 1.0 / a.fs;
    return a;
}
__device__ __forceinline__ void tap_range(const Axis& a, int in, int xx, double& center, int& xmin, int& cnt) {
    center = 0.0 + ((double)xx + 0.5) * a.scale;
    xmin = (int)(center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + a.support + 0.5);
    if (xmax > in) xmax = in;
    cnt = xmax - xmin;
}
template <bool CUBIC>
__device__ __forceinline__ double weight(const Axis& a, int i, int xmin, double center) {
    const double x = ((double)(i + xmin) - center + 0.5) * a.ss;
    return CUBIC ? cubic(x) : tri(x);
}
// normalize_coeffs_8bpc: negative (cubic) weights round towards -inf by half a step
__device__ __forceinline__ int fixed_coeff(double w, double ww) {
    if (ww != 0.0) w = w / ww;
    return w < 0 ? (int)(-0.5 + w * (double)(1 << PB)) : (int)(0.5 + w * (double)(1 << PB));
}
__device__ __forceinline__ int clip8(int v) {
    v >>= PB;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// sequential byte reader over one source row: each aligned word is loaded once
struct Bytes {
    const uint32_t* w;
    long cur;
    uint32_t val;
    __device__ __forceinline__ int at(long q) {
        const long d = q >> 2;
        if (d != cur) {
            cur = d;
            val = w[d];
        }
        return (int)((val >> (8 * (int)(q & 3))) & 255u);
    }
};

struct Norm3 {
    float mean[3], stdv[3];
};

// R x CH: the crop window (columns x rows; the square R x R of the transforms, or the whole resized image of
// pdmk_image_resize_u8).  U8: the resampled bytes themselves go out as HWC uint8 instead of the normalised NCHW floats.
template <int PER, bool CUBIC, bool U8>
__global__ __launch_bounds__(NT) void image_prep_kernel(const uint8_t* __restrict__ src, const pdmk_image_desc* __restrict__ descs,
                                                        int R, int CH, Norm3 nm, float* __restrict__ out,
                                                        uint8_t* __restrict__ out8) {
    __shared__ double h_center[RMAX], h_ww[RMAX];
    __shared__ int h_min[RMAX], h_cnt[RMAX];
    __shared__ int v_k[BAND][KVMAX];
    __shared__ int v_min[BAND], v_cnt[BAND];
    __shared__ uint8_t stage[STAGE_BYTES];

    const int img = blockIdx.y;
    const int y0 = blockIdx.x * BAND;
    const int nb = CH - y0 < BAND ? CH - y0 : BAND;          // output rows of this band
    const pdmk_image_desc d = descs[img];
    const int H = (int)d.h, W = (int)d.w, RH = (int)d.rh, RW = (int)d.rw, top = (int)d.top, left = (int)d.left;
    const Axis ax = make_axis<CUBIC>(W, RW), ay = make_axis<CUBIC>(H, RH);

    // horizontal coefficients of the R crop columns: the weight sum is a sequential double sum, one thread per column
    for (int x = threadIdx.x; x < R; x += NT) {
        double c;
        int m, n;
        tap_range(ax, W, left + x, c, m, n);
        double ww = 0.0;
        for (int i = 0; i < n; ++i) ww += weight<CUBIC>(ax, i, m, c);
        h_center[x] = c;
        h_ww[x] = ww;
        h_min[x] = m;
        h_cnt[x] = n;
    }
    // vertical coefficients of the band's rows, one thread per row
    if (threadIdx.x < nb) {
        const int y = threadIdx.x;
        double c;
        int m, n;
        tap_range(ay, H, top + y0 + y, c, m, n);
        double ww = 0.0;
        for (int i = 0; i < n; ++i) ww += weight<CUBIC>(ay, i, m, c);
        for (int i = 0; i < n; ++i) v_k[y][i] = fixed_coeff(weight<CUBIC>(ay, i, m, c), ww);
        v_min[y] = m;
        v_cnt[y] = n;
    }
    __syncthreads();

    int s0 = v_min[0], s1 = 0;
    for (int y = 0; y < nb; ++y) s1 = max(s1, v_min[y] + v_cnt[y]);
    const int rows_per_chunk = STAGE_BYTES / (3 * R);
    const long row_bytes = 3L * W;
    Bytes rd{reinterpret_cast<const uint32_t*>(src), -1, 0u};

    int acc[PER][3];
#pragma unroll
    for (int j = 0; j < PER; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << (PB - 1);

    for (int c0 = s0; c0 < s1; c0 += rows_per_chunk) {
        const int c1 = min(c0 + rows_per_chunk, s1);
        // horizontal pass of source rows [c0, c1) over the crop columns -> stage[row][channel][x]
        for (int p = threadIdx.x; p < (c1 - c0) * R; p += NT) {
            const int r = p / R, x = p - r * R;
            const int m = h_min[x], n = h_cnt[x];
            const double c = h_center[x], ww = h_ww[x];
            long q = d.offset + (long)(c0 + r) * row_bytes + 3L * m;
            int s[3] = {1 << (PB - 1), 1 << (PB - 1), 1 << (PB - 1)};
            for (int i = 0; i < n; ++i, q += 3) {
                const int k = fixed_coeff(weight<CUBIC>(ax, i, m, c), ww);
                s[0] += rd.at(q) * k;
                s[1] += rd.at(q + 1) * k;
                s[2] += rd.at(q + 2) * k;
            }
            uint8_t* st = stage + (long)r * 3 * R + x;
            st[0] = (uint8_t)clip8(s[0]);
            st[R] = (uint8_t)clip8(s[1]);
            st[2 * R] = (uint8_t)clip8(s[2]);
        }
        __syncthreads();
        // vertical accumulation of the staged rows into this thread's outputs
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int p = threadIdx.x + j * NT;
            const int y = p / R, x = p - y * R;
            if (y < nb) {
                const int m = v_min[y];
                const int lo = max(c0, m), hi = min(c1, m + v_cnt[y]);
                for (int sr = lo; sr < hi; ++sr) {
                    const int k = v_k[y][sr - m];
                    const uint8_t* st = stage + (long)(sr - c0) * 3 * R + x;
                    acc[j][0] += (int)st[0] * k;
                    acc[j][1] += (int)st[R] * k;
                    acc[j][2] += (int)st[2 * R] * k;
                }
            }
        }
        __syncthreads();
    }

    if constexpr (U8) {
        uint8_t* o8 = out8 + (long)img * CH * R * 3;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int p = threadIdx.x + j * NT;
            const int y = p / R, x = p - y * R;
            if (y < nb) {
                uint8_t* q = o8 + ((long)(y0 + y) * R + x) * 3;
                q[0] = (uint8_t)clip8(acc[j][0]);
                q[1] = (uint8_t)clip8(acc[j][1]);
                q[2] = (uint8_t)clip8(acc[j][2]);
            }
        }
        return;
    }
    // ToTensor + Normalize, NCHW fp32; the flip mirrors the crop's columns
    const long plane = (long)R * CH;
    float* o = out + (long)img * 3 * plane;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int p = threadIdx.x + j * NT;
        const int y = p / R, x = p - y * R;
        if (y < nb) {
            const long at = (long)(y0 + y) * R + (d.flip ? R - 1 - x : x);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float v = __fdiv_rn((float)clip8(acc[j][ch]), 255.0f);
                o[ch * plane + at] = __fdiv_rn(__fsub_rn(v, nm.mean[ch]), nm.stdv[ch]);
            }
        }
    }
}

bool desc_ok(const pdmk_image_desc& d, int R, int RH, int64_t src_bytes, int filter) {
    const int64_t lim = 1 << 20;
    if (d.h < 1 || d.w < 1 || d.rh < 1 || d.rw < 1 || d.h > lim || d.w > lim || d.rh > lim || d.rw > lim) return false;
    if (d.top < 0 || d.left < 0 || d.top + RH > d.rh || d.left + R > d.rw) return false;
    if (d.flip != 0 && d.flip != 1) return false;
    if ((d.h + d.rh - 1) / d.rh > (KVMAX - 1) / (filter ? 4 : 2)) return false;   // vertical taps of one output row fit v_k
    if (d.offset < 0 || d.h * d.w * 3 > src_bytes) return false;
    const int64_t end = d.offset + d.h * d.w * 3;
    return end <= src_bytes && ((end + 3) & ~int64_t(3)) <= src_bytes;   // the last aligned word is inside the buffer
}

template <bool CUBIC, bool U8 = false>
void launch(const uint8_t* src, const pdmk_image_desc* desc_dev, int B, int R, int RH, const Norm3& nm, float* out, uint8_t* out8,
            hipStream_t st) {
    const int per = (BAND * R + NT - 1) / NT;
    dim3 grid((unsigned)((RH + BAND - 1) / BAND), (unsigned)B);
    if (per <= 1) hipLaunchKernelGGL((image_prep_kernel<1, CUBIC, U8>), grid, dim3(NT), 0, st, src, desc_dev, R, RH, nm, out, out8);
    else if (per <= 2) hipLaunchKernelGGL((image_prep_kernel<2, CUBIC, U8>), grid, dim3(NT), 0, st, src, desc_dev, R, RH, nm, out, out8);
    else if (per <= 4) hipLaunchKernelGGL((image_prep_kernel<4, CUBIC, U8>), grid, dim3(NT), 0, st, src, desc_dev, R, RH, nm, out, out8);
    else if (per <= 8) hipLaunchKernelGGL((image_prep_kernel<8, CUBIC, U8>), grid, dim3(NT), 0, st, src, desc_dev, R, RH, nm, out, out8);
    else hipLaunchKernelGGL((image_prep_kernel<16, CUBIC, U8>), grid, dim3(NT), 0, st, src, desc_dev, R, RH, nm, out, out8);
}

// torch's CPU upsample_bilinear2d (align_corners=False, no antialiasing) source coordinate: ONE rounding of scale * (dst + 0.5)
// - 0.5 (an explicit fma; nothing else in this file may fuse), clamped at 0; first tap, second tap and the second tap's weight
__device__ __forceinline__ void lerp_axis(int in, float scale, int dst, int& i0, int& i1, float& lam) {
    float s = fmaf(scale, (float)dst + 0.5f, -0.5f);
    if (s < 0.f) s = 0.f;
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + 1 < in ? i0 + 1 : in - 1;
    lam = s - (float)i0;
    lam = lam < 0.f ? 0.f : (lam > 1.f ? 1.f : lam);
}

// one thread per output pixel (3 channels): out[b][y][x][c] = 2 * (clip(bilinear, 0, 255) / 255) - 1, fp32 NHWC
__global__ __launch_bounds__(NT) void resize_bilinear_kernel(const uint8_t* __restrict__ src, const pdmk_image_desc* __restrict__ descs,
                                                             int B, int S, float* __restrict__ out) {
    const long n = (long)B * S * S;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const int b = (int)(i / ((long)S * S)), p = (int)(i - (long)b * S * S);
        const int y = p / S, x = p - y * S;
        const pdmk_image_desc d = descs[b];
        const int H = (int)d.h, W = (int)d.w;
        int x0, x1, y0, y1;
        float lx, ly;
        lerp_axis(W, (float)W / (float)S, x, x0, x1, lx);
        lerp_axis(H, (float)H / (float)S, y, y0, y1, ly);
        const float wx0 = 1.0f - lx, wy0 = 1.0f - ly;
        const uint8_t* r0 = src + d.offset + (long)y0 * W * 3;
        const uint8_t* r1 = src + d.offset + (long)y1 * W * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t = wx0 * (float)r0[3 * x0 + c] + lx * (float)r0[3 * x1 + c];
            const float u = wx0 * (float)r1[3 * x0 + c] + lx * (float)r1[3 * x1 + c];
            float v = wy0 * t + ly * u;
            v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
            out[i * 3 + c] = 2.0f * (v / 255.0f) - 1.0f;
        }
    }
}

}  // namespace

extern "C" int pdmk_image_prep_ex(const uint8_t* src, int64_t src_bytes, const pdmk_image_desc* desc,
                                  const pdmk_image_desc* desc_dev, int B, int R, int filter, const float* mean,
                                  const float* stdv, float* out, pdmk_stream stream) {
    if (!src || !desc || !desc_dev || !out || !mean || !stdv || B < 1 || B > 65535 || R < 1 || R > RMAX || src_bytes < 1 ||
        (filter != 0 && filter != 1) || ((uintptr_t)src & 3) || ((uintptr_t)desc_dev & 7) || ((uintptr_t)out & 3))
        return -1;
    Norm3 nm;
    for (int c = 0; c < 3; ++c) {
        if (!(stdv[c] != 0.0f)) return -1;
        nm.mean[c] = mean[c];
        nm.stdv[c] = stdv[c];
    }
    for (int i = 0; i < B; ++i)
        if (!desc_ok(desc[i], R, R, src_bytes, filter)) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (filter) launch<true>(src, desc_dev, B, R, R, nm, out, nullptr, st);
    else launch<false>(src, desc_dev, B, R, R, nm, out, nullptr, st);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_image_prep(const uint8_t* src, int64_t src_bytes, const pdmk_image_desc* desc,
                               const pdmk_image_desc* desc_dev, int B, int R, float* out, pdmk_stream stream) {
    const float half[3] = {0.5f, 0.5f, 0.5f};
    return pdmk_image_prep_ex(src, src_bytes, desc, desc_dev, B, R, 0, half, half, out, stream);
}

extern "C" int pdmk_image_resize_u8(const uint8_t* src, int64_t src_bytes, const pdmk_image_desc* desc,
                                    const pdmk_image_desc* desc_dev, int B, int OH, int OW, uint8_t* out, pdmk_stream stream) {
    if (!src || !desc || !desc_dev || !out || B < 1 || B > 65535 || OH < 1 || OW < 1 || OW > RMAX || OH > (1 << 20) ||
        src_bytes < 1 || ((uintptr_t)src & 3) || ((uintptr_t)desc_dev & 7))
        return -1;
    for (int i = 0; i < B; ++i) {
        const pdmk_image_desc& d = desc[i];
        if (d.rh != OH || d.rw != OW || d.top != 0 || d.left != 0 || d.flip != 0 || !desc_ok(d, OW, OH, src_bytes, 1)) return -1;
    }
    launch<true, true>(src, desc_dev, B, OW, OH, Norm3{}, nullptr, out, (hipStream_t)stream);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_resize_bilinear_u8(const uint8_t* src, int64_t src_bytes, const pdmk_image_desc* desc,
                                       const pdmk_image_desc* desc_dev, int B, int S, float* out, pdmk_stream stream) {
    if (!src || !desc || !desc_dev || !out || B < 1 || S < 1 || S > (1 << 14) || src_bytes < 1 || ((uintptr_t)desc_dev & 7) ||
        ((uintptr_t)out & 3))
        return -1;
    const int64_t lim = 1 << 20;
    for (int i = 0; i < B; ++i) {
        const pdmk_image_desc& d = desc[i];
        if (d.h < 1 || d.w < 1 || d.h > lim || d.w > lim || d.offset < 0 || d.h * d.w * 3 > src_bytes ||
            d.offset + d.h * d.w * 3 > src_bytes)
            return -1;
    }
    const long g = ((long)B * S * S + NT - 1) / NT;
    hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)(g < 65536 ? g : 65536)), dim3(NT), 0, (hipStream_t)stream, src,
                       desc_dev, B, S, out);
    PDMK_CHECK_LAUNCH();
    return 0;
}
