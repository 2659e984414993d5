// The classifier head of the object-erasure evaluation (pdm/models/resnet): top-k of softmax(logits) on the device.
//   pdmk_softmax_topk : logits fp32 [B, N] (row stride ld) -> probs fp32 [B, k], idx int32 [B, k], k <= 16, N <= 65536.
// and CLIP's zero-shot head of the debiasing baseline (pdm/utils/uce_debias.py), further down:
//   pdmk_zeroshot_head : image features [B, D], class-text features [A, D] -> softmax probs, "which class wins" mask, counts.
//
// One wave per row, four rows per workgroup; lane l owns the columns l, l + 64, l + 128, ... (coalesced 256-byte reads).  With
// N <= 1024 the lane's 16 values stay in registers for all three steps, otherwise each step reads the row again:
//   1. row maximum (NaN skipped) by xor-shuffle reduction;
//   2. sum exp(x - max) in fp32: each lane adds its elements in column order, then the xor-shuffle tree - one fixed order;
//   3. k rounds of a wave arg-max.  Every element has a 64-bit key (ordered value bits, 0xffffffff - column): a larger key is
//      a larger value or, between equal values, a lower column; a NaN's value bits are all ones, so it outranks everything and
//      NaNs come lower column first.  The keys of a row are distinct, so round j takes the largest key below round j - 1's
//      winner - no taken-mask.  Only the k winners are divided by the sum.
// A NaN in the row makes the sum, and with it every probability, NaN.  No atomics, no LDS: two launches give the same bits.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int REG_E = 16;                  // elements a lane keeps in registers: rows of up to 64 * 16 columns

// ordered key of a value: unsigned order == float order, -0 counted as +0, NaN above +inf
__device__ __forceinline__ unsigned value_key(float x) {
    if (x != x) return 0xffffffffu;
    unsigned u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);      // all ones -> 0x7fffffff, a NaN
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        v = other > v ? other : v;
    }
    return v;
}

template <bool REG>
__global__ __launch_bounds__(NT) void softmax_topk_kernel(const float* __restrict__ logits, int ld, int B, int N, int k,
                                                          float* __restrict__ probs, int* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (row >= B) return;                                   // whole waves leave: the shuffles below see full waves
    const float* x = logits + (long)row * ld;
    const int ne = REG ? REG_E : (N + 63) / 64;

    float v[REG ? REG_E : 1];
    if constexpr (REG) {
#pragma unroll
        for (int e = 0; e < REG_E; ++e) {
            const int c = lane + 64 * e;
            v[e] = c < N ? x[c] : -INFINITY;
        }
    }
    auto at = [&](int e) { return x[lane + 64 * e]; };      // the re-reading form's element e of this lane

    float mx = -INFINITY;
    if constexpr (REG) {
#pragma unroll
        for (int e = 0; e < REG_E; ++e) mx = fmaxf(mx, v[e]);
    } else {
        for (int e = 0; e < ne; ++e)
            if (lane + 64 * e < N) mx = fmaxf(mx, at(e));
    }
    mx = wave_max(mx);

    float s = 0.f;
    if constexpr (REG) {
#pragma unroll
        for (int e = 0; e < REG_E; ++e)
            if (lane + 64 * e < N) s += expf(v[e] - mx);
    } else {
        for (int e = 0; e < ne; ++e)
            if (lane + 64 * e < N) s += expf(at(e) - mx);
    }
    s = wave_sum(s);

    unsigned long long prev = 0;
    float myp = 0.f;
    int myi = 0;
    for (int j = 0; j < k; ++j) {
        unsigned long long best = 0;                        // 0 is below every element's key (its low word is >= 0xffff0000)
        auto offer = [&](int e, float val) {
            const int c = lane + 64 * e;
            const unsigned long long key = ((unsigned long long)value_key(val) << 32) | (0xffffffffu - (unsigned)c);
            if (c < N && (j == 0 || key < prev) && key > best) best = key;
        };
        if constexpr (REG) {
#pragma unroll
            for (int e = 0; e < REG_E; ++e) offer(e, v[e]);
        } else {
            for (int e = 0; e < ne; ++e)
                if (lane + 64 * e < N) offer(e, at(e));
        }
        best = wave_max_u64(best);
        prev = best;
        if (lane == j) {
            myp = expf(key_value((unsigned)(best >> 32)) - mx) / s;
            myi = (int)(0xffffffffu - (unsigned)best);
        }
    }
    if (lane < k) {
        probs[(long)row * k + lane] = myp;
        idx[(long)row * k + lane] = myi;
    }
}

// One wave per image row, four rows per workgroup; lane l owns the columns l, l + 64, ... of the feature rows (coalesced
// 256-byte reads; the image row is read again per class, from cache).  Sums in fp64: each lane adds its columns in order, then
// the xor butterfly, which leaves the same bits in every lane.  Lane a keeps class a's logit, so the row maximum, the softmax
// sum and the mask are one value per lane; lanes from A on hold -inf / 0.  The softmax of the fp32 logits is evaluated in fp64
// and rounded once, so what separates it from torch's fp32 evaluation of the same formula is torch's own rounding.
__global__ __launch_bounds__(NT) void zeroshot_head_kernel(const float* __restrict__ img, int lda, const float* __restrict__ txt,
                                                           int ldb, int B, int A, int D, float scale, float* __restrict__ probs,
                                                           int* __restrict__ mask, const int* __restrict__ group,
                                                           int* __restrict__ hits, int G) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (row >= B) return;                                   // whole waves leave: the shuffles below see full waves
    const float* x = img + (long)row * lda;
    double xx = 0.0;
    for (int c = lane; c < D; c += 64) {
        const double v = (double)x[c];
        xx = fma(v, v, xx);
    }
    xx = wave_sum_d(xx);
    float logit = -INFINITY;
    for (int a = 0; a < A; ++a) {
        const float* t = txt + (long)a * ldb;
        double d = 0.0, tt = 0.0;
        for (int c = lane; c < D; c += 64) {
            const double v = (double)x[c], u = (double)t[c];
            d = fma(v, u, d);
            tt = fma(u, u, tt);
        }
        d = wave_sum_d(d);
        tt = wave_sum_d(tt);
        const double den = sqrt(xx) * sqrt(tt);
        const double cs = den > 0.0 ? d / den : 0.0;
        const float z = (float)((double)scale * cs);
        if (lane == a) logit = z;
    }
    const float mx = wave_max(logit);
    const double e = lane < A ? exp((double)(logit - mx)) : 0.0;      // the fp32 difference, as torch forms it
    const double s = wave_sum_d(e);
    if (lane < A) {
        const int hit = logit == mx ? 1 : 0;
        probs[(long)row * A + lane] = (float)(e / s);
        mask[(long)row * A + lane] = hit;
        if (hits && hit) {
            const int g = group ? group[row] : 0;
            if (g >= 0 && g < G) atomicAdd(&hits[(long)g * A + lane], 1);
        }
    }
}

}  // namespace

extern "C" int pdmk_softmax_topk(const float* logits, int ld, int B, int N, int k, float* probs, int* idx, pdmk_stream stream) {
    if (!logits || !probs || !idx || ((uintptr_t)logits & 3) || ((uintptr_t)probs & 3) || ((uintptr_t)idx & 3) || B < 1 ||
        B > (1 << 24) || N < 1 || N > 65536 || k < 1 || k > 16 || k > N || ld < N)
        return -1;
    const dim3 grid((unsigned)((B + NT / 64 - 1) / (NT / 64)));
    hipStream_t st = (hipStream_t)stream;
    if (N <= 64 * REG_E) hipLaunchKernelGGL(softmax_topk_kernel<true>, grid, dim3(NT), 0, st, logits, ld, B, N, k, probs, idx);
    else hipLaunchKernelGGL(softmax_topk_kernel<false>, grid, dim3(NT), 0, st, logits, ld, B, N, k, probs, idx);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_zeroshot_head(const float* img, int lda, const float* txt, int ldb, int B, int A, int D, float scale,
                                  float* probs, int* mask, const int* group, int* hits, int G, pdmk_stream stream) {
    if (!img || !txt || !probs || !mask ||
        (((uintptr_t)img | (uintptr_t)txt | (uintptr_t)probs | (uintptr_t)mask | (uintptr_t)group | (uintptr_t)hits) & 3) || B < 1 ||
        B > 65535 || A < 1 || A > PDMK_ZEROSHOT_MAX_CLASSES || D < 1 || D > 4096 || lda < D || ldb < D || (hits && G < 1))
        return -1;
    const dim3 grid((unsigned)((B + NT / 64 - 1) / (NT / 64)));
    hipLaunchKernelGGL(zeroshot_head_kernel, grid, dim3(NT), 0, (hipStream_t)stream, img, lda, txt, ldb, B, A, D, scale, probs,
                       mask, group, hits, G);
    PDMK_CHECK_LAUNCH();
    return 0;
}
