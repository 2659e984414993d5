// Kernels of the CLIP score (OpenAI CLIP ViT image tower + text tower + cosine head) that have no counterpart in the
// U-Net / VAE / text-conditioning paths; LayerNorm, the projections and attention run on the existing entry points.
//   pdmk_patch_im2col   : ViT patch embedding's stride-p conv as a GEMM operand, rows (b, gy, gx), cols (c, ky, kx).
//   pdmk_vit_tokens     : [CLS | patches] + position embedding.
//   pdmk_quick_gelu_fwd : x * sigmoid(1.702 x) (transformers' QuickGELUActivation, OpenAI CLIP's MLP activation).
//   pdmk_gather_rows    : one row per sequence: row 0 (CLS) or the row at the first argmax of the token ids (EOT).
//   pdmk_clip_score_head: row L2 normalisation in fp32 and the sum of the per-row cosines into an fp64 accumulator.
// tests/test_encoder_forms_gpu.py restates grid_for's cap (8192) and test_restated_constants_are_the_sources matches it against
// this text: change the two together.
#include "vec.h"

namespace {

constexpr int NT = 256;

template <typename T>
__global__ __launch_bounds__(NT) void im2col_kernel(const float* __restrict__ x, T* __restrict__ out, int B, int S, int p,
                                                    int ldo) {
    const int g = S / p, K = 3 * p * p;
    const long n = (long)B * g * g * ldo;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const long r = i / ldo;
        const int c = (int)(i - r * ldo);
        float v = 0.f;
        if (c < K) {
            const int b = (int)(r / ((long)g * g)), pi = (int)(r - (long)b * g * g);
            const int gy = pi / g, gx = pi - gy * g;
            const int ch = c / (p * p), kk = c - ch * p * p;
            const int ky = kk / p, kx = kk - ky * p;
            v = x[(((long)b * 3 + ch) * S + gy * p + ky) * S + gx * p + kx];
        }
        out[i] = from_f32<T>(v);
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void vit_tokens_kernel(const T* __restrict__ patches, int ldp, const T* __restrict__ cls,
                                                        const T* __restrict__ pos, int ldpos, T* __restrict__ out, int ldo,
                                                        int B, int G2, int E) {
    const int N = G2 + 1;
    const long n = (long)B * N * E;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const long r = i / E;
        const int c = (int)(i - r * E);
        const int b = (int)(r / N), t = (int)(r - (long)b * N);
        const float a = t == 0 ? to_f32(cls[c]) : to_f32(patches[((long)b * G2 + t - 1) * ldp + c]);
        out[r * ldo + c] = from_f32<T>(a + to_f32(pos[(long)t * ldpos + c]));
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void quick_gelu_kernel(const T* __restrict__ x, T* __restrict__ y, long n) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const float v = to_f32(x[i]);
        y[i] = from_f32<T>(v * (1.0f / (1.0f + expf(-(1.702f * v)))));
    }
}

// one workgroup per sequence: the first maximum of its ids (a serial scan: T is the context length, 77), then the row copy
template <typename T>
__global__ __launch_bounds__(NT) void gather_rows_kernel(const T* __restrict__ x, int ldx, const int64_t* __restrict__ ids,
                                                         int T_, T* __restrict__ out, int ldo, int D) {
    __shared__ int pick;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        int best = 0;
        if (ids) {
            const int64_t* row = ids + (long)b * T_;
            int64_t m = row[0];
            for (int t = 1; t < T_; ++t)
                if (row[t] > m) {
                    m = row[t];
                    best = t;
                }
        }
        pick = best;
    }
    __syncthreads();
    const T* src = x + ((long)b * T_ + pick) * ldx;
    for (int c = threadIdx.x; c < D; c += NT) out[(long)b * ldo + c] = src[c];
}

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// one workgroup per row: an = a / |a|, bn = b / |b| (fp32), acc += sum(an * bn) (fp64)
__global__ __launch_bounds__(NT) void score_head_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b,
                                                        int ldb, float* __restrict__ an, float* __restrict__ bn,
                                                        double* __restrict__ acc, int D) {
    __shared__ float red[NT / 64];
    const long r = blockIdx.x;
    const float* ar = a + r * lda;
    float s = 0.f;
    for (int c = threadIdx.x; c < D; c += NT) s += ar[c] * ar[c];
    const float na = sqrtf(block_sum(s, red));
    if (an)
        for (int c = threadIdx.x; c < D; c += NT) an[r * D + c] = ar[c] / na;
    if (!b) return;
    const float* br = b + r * ldb;
    s = 0.f;
    for (int c = threadIdx.x; c < D; c += NT) s += br[c] * br[c];
    const float nb = sqrtf(block_sum(s, red));
    float dot = 0.f;
    for (int c = threadIdx.x; c < D; c += NT) {
        const float u = ar[c] / na, v = br[c] / nb;
        if (bn) bn[r * D + c] = v;
        dot += u * v;
    }
    dot = block_sum(dot, red);
    if (threadIdx.x == 0 && acc) atomicAdd(acc, (double)dot);
}

// one workgroup per row: sim_a = cos(t, a), sim_b = cos(t, b) with every norm clamped below at 1e-8 (a zero row gives 0),
// b_lt_a = the comparison of the two stored fp32 values.  Fixed reduction order, no atomics: a row's result does not depend on
// the batch it is in.
__global__ __launch_bounds__(NT) void cosine_pairs_kernel(const float* __restrict__ t, int ldt, const float* __restrict__ a,
                                                          int lda, const float* __restrict__ b, int ldb,
                                                          float* __restrict__ sim_a, float* __restrict__ sim_b,
                                                          int32_t* __restrict__ b_lt_a, int D) {
    __shared__ float red[NT / 64];
    const long r = blockIdx.x;
    const float *tr = t + r * ldt, *ar = a + r * lda, *br = b + r * ldb;
    float tt = 0.f, aa = 0.f, bb = 0.f, ta = 0.f, tb = 0.f;
    for (int c = threadIdx.x; c < D; c += NT) {
        const float x = tr[c], u = ar[c], v = br[c];
        tt += x * x;
        aa += u * u;
        bb += v * v;
        ta += x * u;
        tb += x * v;
    }
    tt = block_sum(tt, red);
    aa = block_sum(aa, red);
    bb = block_sum(bb, red);
    ta = block_sum(ta, red);
    tb = block_sum(tb, red);
    if (threadIdx.x == 0) {
        const float eps = 1e-8f;
        const float nt = fmaxf(sqrtf(tt), eps), na = fmaxf(sqrtf(aa), eps), nb = fmaxf(sqrtf(bb), eps);
        const float sa = ta / nt / na, sb = tb / nt / nb;
        sim_a[r] = sa;
        sim_b[r] = sb;
        b_lt_a[r] = sb < sa ? 1 : 0;
    }
}

unsigned grid_for(long n) {
    const long g = (n + NT - 1) / NT;
    return (unsigned)(g < 8192 ? g : 8192);
}

template <typename T> int im2col_launch(const float* x, void* out, int B, int S, int p, int ldo, hipStream_t st) {
    const long n = (long)B * (S / p) * (S / p) * ldo;
    hipLaunchKernelGGL(im2col_kernel<T>, dim3(grid_for(n)), dim3(NT), 0, st, x, (T*)out, B, S, p, ldo);
    PDMK_CHECK_LAUNCH();
    return 0;
}

template <typename T>
int tokens_launch(const void* patches, int ldp, const void* cls, const void* pos, int ldpos, void* out, int ldo, int B, int G2,
                  int E, hipStream_t st) {
    hipLaunchKernelGGL(vit_tokens_kernel<T>, dim3(grid_for((long)B * (G2 + 1) * E)), dim3(NT), 0, st, (const T*)patches, ldp,
                       (const T*)cls, (const T*)pos, ldpos, (T*)out, ldo, B, G2, E);
    PDMK_CHECK_LAUNCH();
    return 0;
}

template <typename T> int quick_gelu_launch(const void* x, void* y, long n, hipStream_t st) {
    hipLaunchKernelGGL(quick_gelu_kernel<T>, dim3(grid_for(n)), dim3(NT), 0, st, (const T*)x, (T*)y, n);
    PDMK_CHECK_LAUNCH();
    return 0;
}

template <typename T>
int gather_launch(const void* x, int ldx, const int64_t* ids, int T_, void* out, int ldo, int B, int D, hipStream_t st) {
    hipLaunchKernelGGL(gather_rows_kernel<T>, dim3(B), dim3(NT), 0, st, (const T*)x, ldx, ids, T_, (T*)out, ldo, D);
    PDMK_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int pdmk_patch_im2col(const float* x, void* out, int B, int S, int p, int ldo, int dtype, pdmk_stream stream) {
    if (!x || !out || B <= 0 || p <= 0 || S < p || S % p || ldo < 3 * p * p) return -1;
    PDMK_DISPATCH(dtype, im2col_launch, x, out, B, S, p, ldo, (hipStream_t)stream);
}

extern "C" int pdmk_vit_tokens(const void* patches, int ldp, const void* cls, const void* pos, int ldpos, void* out, int ldo,
                               int B, int G2, int E, int dtype, pdmk_stream stream) {
    if (!patches || !cls || !pos || !out || B <= 0 || G2 <= 0 || E <= 0 || ldp < E || ldpos < E || ldo < E) return -1;
    PDMK_DISPATCH(dtype, tokens_launch, patches, ldp, cls, pos, ldpos, out, ldo, B, G2, E, (hipStream_t)stream);
}

extern "C" int pdmk_quick_gelu_fwd(const void* x, void* y, int64_t n, int dtype, pdmk_stream stream) {
    if (!x || !y || n <= 0) return -1;
    PDMK_DISPATCH(dtype, quick_gelu_launch, x, y, (long)n, (hipStream_t)stream);
}

extern "C" int pdmk_gather_rows(const void* x, int ldx, const int64_t* ids, int T, void* out, int ldo, int B, int D,
                                int dtype, pdmk_stream stream) {
    if (!x || !out || B <= 0 || B > 65535 || T <= 0 || D <= 0 || ldx < D || ldo < D) return -1;
    PDMK_DISPATCH(dtype, gather_launch, x, ldx, ids, T, out, ldo, B, D, (hipStream_t)stream);
}

extern "C" int pdmk_clip_score_head(const float* a, int lda, const float* b, int ldb, float* an, float* bn, double* acc,
                                    int B, int D, pdmk_stream stream) {
    if (!a || B <= 0 || B > 65535 || D <= 0 || lda < D || (b && ldb < D) || (!b && (bn || acc)) || (!an && !b)) return -1;
    hipLaunchKernelGGL(score_head_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, a, lda, b, ldb, an, bn, acc, D);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_cosine_pairs(const float* t, int ldt, const float* a, int lda, const float* b, int ldb, float* sim_a,
                                 float* sim_b, int32_t* b_lt_a, int B, int D, pdmk_stream stream) {
    if (!t || !a || !b || !sim_a || !sim_b || !b_lt_a || B <= 0 || B > 65535 || D <= 0 || ldt < D || lda < D || ldb < D)
        return -1;
    hipLaunchKernelGGL(cosine_pairs_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, t, ldt, a, lda, b, ldb, sim_a, sim_b,
                       b_lt_a, D);
    PDMK_CHECK_LAUNCH();
    return 0;
}
