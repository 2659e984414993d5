// ConceptPrune / Wanda kernels (include/pdmk.h "ConceptPrune"): the observation step on the GEGLU output that feeds ff.net.2
// (row-normalised squared column sums), the per-row top-k selection of |W| * norm scores over all timesteps (as counts over time,
// or as one bit per timestep and weight), the time-averaged mask, and the per-timestep masks applied to the compute weights.
//
// Everything here is reproducible bit for bit from launch to launch: masks are built on comparisons of these numbers, so no
// float atomics anywhere - sums go through wave butterflies, LDS and partial slabs in a fixed order.
#include "vec.h"

namespace {

constexpr int NT = 256;

// ---------------------------------------------------------------------------------------------------- observation
// Pass 1: inv[m] = max(||x[m, :]||_2, 1e-12), the divisor of F.normalize: one wave per row (4 rows per workgroup), 8 elements
// per lane and step.
template <typename T>
__device__ __forceinline__ void load8(const T* p, float* f) {
    if constexpr (std::is_same<T, bf16>::value) {
        Vec<bf16>::load(p, f);
    } else {
        Vec<float>::load(p, f);
        Vec<float>::load(p + 4, f + 4);
    }
}

template <typename T>
__global__ void __launch_bounds__(NT) rowinv_kernel(const T* __restrict__ x, int M, int F, int ld, float* __restrict__ inv) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (row >= M) return;                                     // whole waves leave: the butterfly below sees full waves
    const T* xr = x + (long)row * ld;
    float ss = 0.f;
    for (int c = lane * 8; c < F; c += 64 * 8) {
        float f[8];
        load8(xr + c, f);
#pragma unroll
        for (int i = 0; i < 8; ++i) ss = fmaf(f[i], f[i], ss);
    }
    ss = wave_sum(ss);
    if (lane == 0) inv[row] = fmaxf(sqrtf(ss), 1e-12f);
}

// Pass 2: workgroup (column chunk cx, row block ry): part[ry][c] = sum over the block's rows of (x[m][c] / inv[m])^2 for the
// chunk's 256 columns.  Thread = (row lane rl of 8, column group cg of 32, 8 columns): a row lane reads 512 B (bf16) / 1 KiB
// (fp32) contiguous per row.  The 8 row lanes are added in order through LDS.  A true division, as F.normalize does it (one
// rounding per element; the kernel stays bound by its reads).
constexpr int CW = 256;            // columns per chunk
constexpr int RL = 8;              // row lanes
template <typename T>
__global__ void __launch_bounds__(NT) colsq_part_kernel(const T* __restrict__ x, int M, int F, int ld, const float* __restrict__ inv,
                                                        int rows_per_block, float* __restrict__ part) {
    __shared__ float red[RL][CW];
    const int cg = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * CW + cg * 8;
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = min(M, r0 + rows_per_block);
    float a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = 0.f;
    if (c < F) {                                              // F % 8 == 0: a column group is inside the row or outside it
#pragma unroll 4
        for (int r = r0 + rl; r < r1; r += RL) {
            float f[8];
            load8(x + (long)r * ld + c, f);
            const float s = inv[r];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float v = f[i] / s;
                a[i] = fmaf(v, v, a[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) red[rl][cg * 8 + i] = a[i];
    __syncthreads();
    const int co = blockIdx.x * CW + threadIdx.x;
    if (co < F) {
        float s = red[0][threadIdx.x];
#pragma unroll
        for (int j = 1; j < RL; ++j) s += red[j][threadIdx.x];
        part[(long)blockIdx.y * F + co] = s;
    }
}

// Pass 3: acc[c] += sum over the row blocks, four interleaved running sums combined in a fixed order.
__global__ void __launch_bounds__(NT) colsq_sum_kernel(const float* __restrict__ part, int nrb, int F, float* __restrict__ acc) {
    const int c = blockIdx.x * NT + threadIdx.x;
    if (c >= F) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int b = 0;
    for (; b + 4 <= nrb; b += 4) {
        s0 += part[(long)b * F + c];
        s1 += part[(long)(b + 1) * F + c];
        s2 += part[(long)(b + 2) * F + c];
        s3 += part[(long)(b + 3) * F + c];
    }
    for (; b < nrb; ++b) s0 += part[(long)b * F + c];
    acc[c] += (s0 + s1) + (s2 + s3);
}

// rows per block of pass 2: enough workgroups for every CU at both ends of the shape range (M = 18 432 x F = 1 280: 5 chunks x
// 205 row blocks; M = 128 x F = 5 120: 20 chunks x 16 row blocks), never fewer than one row per row lane
inline int colsq_rows_per_block(int M, int F) {
    const int nchunk = (F + CW - 1) / CW;
    const int want = max(1, 1024 / nchunk);                   // row blocks wanted
    int rpb = (M + want - 1) / want;
    rpb = (rpb + RL - 1) / RL * RL;
    return max(rpb, RL);
}

template <typename T>
int rownorm_colsq_t(const void* x, int M, int F, int ld, float* acc, float* ws, hipStream_t st) {
    const T* xp = (const T*)x;
    const int rpb = colsq_rows_per_block(M, F);
    const int nrb = (M + rpb - 1) / rpb;
    float* inv = ws;
    float* part = ws + ((long)M + 63) / 64 * 64;
    hipLaunchKernelGGL(rowinv_kernel<T>, dim3((M + 3) / 4), dim3(NT), 0, st, xp, M, F, ld, inv);
    hipLaunchKernelGGL(colsq_part_kernel<T>, dim3((F + CW - 1) / CW, nrb), dim3(NT), 0, st, xp, M, F, ld, inv, rpb, part);
    hipLaunchKernelGGL(colsq_sum_kernel, dim3((F + NT - 1) / NT), dim3(NT), 0, st, part, nrb, F, acc);
    PDMK_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------- selection
// fp32 bits -> unsigned key with the order of the values (finite inputs)
__device__ __forceinline__ unsigned order_key(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Sum of one int per thread over the workgroup, the same value in every thread.  `slot` alternates between two LDS buffers, so
// one barrier per call is enough: a wave that is still reading buffer p cannot be overtaken by a write to p, which is two calls
// (one more barrier) away.
__device__ __forceinline__ int block_count(int v, int (*buf)[NT / 64], int& slot) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    int* b = buf[slot];
    slot ^= 1;
    if ((threadIdx.x & 63) == 0) b[threadIdx.x >> 6] = v;
    __syncthreads();
    return b[0] + b[1] + b[2] + b[3];
}

// Where a row's selection goes.  wanda_select_row calls emit(t, j, sel) for every t and j from ALL threads of the workgroup (a
// policy may use wave-wide operations), sel being the outcome for column f = j * 256 + tid (false at f >= F), and finish() once.
// CountOut: count[o][f] += the number of t at which f is selected, kept in registers until the end (pdmk_wanda_count).
template <int NPT>
struct CountOut {
    int32_t* cr;
    int F;
    int cnt[NPT];
    __device__ __forceinline__ CountOut(int32_t* row, int F_) : cr(row), F(F_) {
#pragma unroll
        for (int j = 0; j < NPT; ++j) cnt[j] = 0;
    }
    __device__ __forceinline__ void emit(int, int j, bool sel) { cnt[j] += sel ? 1 : 0; }
    __device__ __forceinline__ void finish() {
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int f = j * NT + (int)threadIdx.x;
            if (f < F) cr[f] += cnt[j];
        }
    }
};
// BitsOut: one bit per (t, f), overwritten (pdmk_wanda_select).  A wave's ballot at j covers the 64 columns from
// j * 256 + wave * 64: exactly the words j * 8 + wave * 2 and the next one, stored by lanes 0 and 32 with plain vector stores.
// Columns at f >= F carry sel = false, so the tail bits of the last word are 0; words past the row are not written.
struct BitsOut {
    uint32_t* row;             // word 0 of row o at t = 0
    long t_stride;
    int row_words;
    __device__ __forceinline__ void emit(int t, int j, bool sel) {
        const unsigned long long m = __ballot(sel);
        const int lane = threadIdx.x & 63;
        const int word = j * (NT / 32) + (int)(threadIdx.x >> 6) * 2 + (lane >> 5);
        if ((lane & 31) == 0 && word < row_words) row[t * t_stride + word] = (uint32_t)(m >> (lane & 32));
    }
    __device__ __forceinline__ void finish() {}
};

// The selection of one weight row by one workgroup; thread tid owns the columns f = j * 256 + tid, j < NPT: |W[o, f]| stays
// in registers across the T timesteps.  The k-th largest score is found by bisection on the 32 key bits (the largest threshold
// that at least k keys reach), one workgroup-wide count per bit and no atomics; keys equal to it are taken in ascending f.
// k <= 0 selects nothing, k >= F the whole row (both still gated by mt > mb and emitted).
template <typename T, int NPT, typename Out>
__device__ __forceinline__ void wanda_select_row(const T* __restrict__ wr, int F, const float* __restrict__ n_base,
                                                 const float* __restrict__ n_target, int nT, int k, Out& out) {
    __shared__ int cbuf[2][NT / 64];
    __shared__ int wtie[NT / 64];
    int slot = 0;
    const int tid = threadIdx.x;
    float aw[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int f = j * NT + tid;
        aw[j] = f < F ? fabsf(to_f32(wr[f])) : 0.f;
    }
    for (int t = 0; t < nT; ++t) {
        const float* nb = n_base + (long)t * F;
        const float* nt = n_target + (long)t * F;
        unsigned key[NPT];
        unsigned gt = 0;                                      // bit j: mt > mb at column j
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int f = j * NT + tid;
            key[j] = 0u;                                      // below the key of every finite value: never selected
            if (f < F) {
                const float mt = aw[j] * nt[f] + 0.0f;        // (-0 -> +0: equal values get equal keys)
                const float mb = aw[j] * nb[f];
                key[j] = order_key(mt);
                gt |= (mt > mb ? 1u : 0u) << j;
            }
        }
        if (k >= F || k <= 0) {                               // the whole row, or nothing
#pragma unroll
            for (int j = 0; j < NPT; ++j) out.emit(t, j, k > 0 && ((gt >> j) & 1u));
            continue;
        }
        unsigned thr = 0u;
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned cand = thr | (1u << bit);
            int c = 0;
#pragma unroll
            for (int j = 0; j < NPT; ++j) c += key[j] >= cand ? 1 : 0;
            if (block_count(c, cbuf, slot) >= k) thr = cand;
        }
        int c = 0;
#pragma unroll
        for (int j = 0; j < NPT; ++j) c += key[j] > thr ? 1 : 0;
        int need = k - block_count(c, cbuf, slot);            // keys equal to thr that are selected: >= 1
        c = 0;
#pragma unroll
        for (int j = 0; j < NPT; ++j) c += key[j] == thr ? 1 : 0;
        const int nties = block_count(c, cbuf, slot);
        if (nties <= need) {                                  // no tie across the k-th place
#pragma unroll
            for (int j = 0; j < NPT; ++j) out.emit(t, j, key[j] >= thr && ((gt >> j) & 1u));
        } else {                                              // the first `need` of them in ascending f = (j, tid)
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const bool tie = key[j] == thr;
                const unsigned long long m = __ballot(tie);
                const int lane = tid & 63, wv = tid >> 6;
                const int before = __popcll(m & ((1ull << lane) - 1ull));
                __syncthreads();                              // the previous round's wtie has been read
                if (lane == 0) wtie[wv] = __popcll(m);
                __syncthreads();
                int base = 0, tot = 0;
#pragma unroll
                for (int q = 0; q < NT / 64; ++q) {
                    base += q < wv ? wtie[q] : 0;
                    tot += wtie[q];
                }
                const bool sel = key[j] > thr || (tie && base + before < need);
                out.emit(t, j, sel && ((gt >> j) & 1u));
                need -= tot;                                  // (may go negative: nothing more is taken)
            }
        }
    }
    out.finish();
}

// One workgroup per weight row o, all T timesteps in the launch.
template <typename T, int NPT>
__global__ void __launch_bounds__(NT) wanda_count_kernel(const T* __restrict__ w, int F, int ldw, const float* __restrict__ n_base,
                                                         const float* __restrict__ n_target, int nT, int k,
                                                         int32_t* __restrict__ count) {
    CountOut<NPT> out(count + (long)blockIdx.x * F, F);
    wanda_select_row<T, NPT>(w + (long)blockIdx.x * ldw, F, n_base, n_target, nT, k, out);
}

template <typename T, int NPT>
__global__ void __launch_bounds__(NT) wanda_select_kernel(const T* __restrict__ w, int F, int ldw, const float* __restrict__ n_base,
                                                          const float* __restrict__ n_target, int nT, int k,
                                                          uint32_t* __restrict__ bits, long t_stride) {
    const int row_words = (F + 31) >> 5;
    BitsOut out{bits + (long)blockIdx.x * row_words, t_stride, row_words};
    wanda_select_row<T, NPT>(w + (long)blockIdx.x * ldw, F, n_base, n_target, nT, k, out);
}

// NPT by width: 5, 10 or 20 columns per thread
#define WANDA_BY_WIDTH(KERNEL, ...)                                                                        \
    do {                                                                                                   \
        if (F <= 5 * NT)                                                                                   \
            hipLaunchKernelGGL((KERNEL<T, 5>), dim3(O), dim3(NT), 0, st, __VA_ARGS__);                     \
        else if (F <= 10 * NT)                                                                             \
            hipLaunchKernelGGL((KERNEL<T, 10>), dim3(O), dim3(NT), 0, st, __VA_ARGS__);                    \
        else                                                                                               \
            hipLaunchKernelGGL((KERNEL<T, 20>), dim3(O), dim3(NT), 0, st, __VA_ARGS__);                    \
    } while (0)

template <typename T>
int wanda_count_t(const void* w, int O, int F, int ldw, const float* nb, const float* nt, int nT, int k, int32_t* count,
                  hipStream_t st) {
    WANDA_BY_WIDTH(wanda_count_kernel, (const T*)w, F, ldw, nb, nt, nT, k, count);
    PDMK_CHECK_LAUNCH();
    return 0;
}

template <typename T>
int wanda_select_t(const void* w, int O, int F, int ldw, const float* nb, const float* nt, int nT, int k, uint32_t* bits,
                   long t_stride, hipStream_t st) {
    WANDA_BY_WIDTH(wanda_select_kernel, (const T*)w, F, ldw, nb, nt, nT, k, bits, t_stride);
    PDMK_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------- mask
template <typename T>
__global__ void __launch_bounds__(NT) wanda_apply_kernel(T* __restrict__ w, int O, int F, int ldw, const int32_t* __restrict__ count,
                                                         float threshold) {
    const long n = (long)O * F;
    for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const int o = (int)(i / F), f = (int)(i - (long)o * F);
        if ((float)count[i] > threshold) w[(long)o * ldw + f] = from_f32<T>(0.f);
    }
}

template <typename T>
int wanda_apply_t(void* w, int O, int F, int ldw, const int32_t* count, float threshold, hipStream_t st) {
    const long n = (long)O * F;
    const int grid = (int)max(1L, min(4096L, (n + NT - 1) / NT));
    hipLaunchKernelGGL(wanda_apply_kernel<T>, dim3(grid), dim3(NT), 0, st, (T*)w, O, F, ldw, count, threshold);
    PDMK_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------- per-timestep masks
// One workgroup per table row (some rows of one layer): dst = bit ? 0 : src over the row's F columns, a select in T.  The slot
// is resolved here, from the host value or from the sampler's device-side call counter, so one captured launch serves every
// step; outside [0, nT), or without bits, the pristine weights are written.  16-byte chunks where F, ld and the two offsets are
// multiples of the chunk (the pointers are 16-byte aligned, checked on the host), else element by element.
template <typename T>
__global__ void __launch_bounds__(NT) masked_weights_kernel(T* __restrict__ dst, const T* __restrict__ src,
                                                            const pdmk_mask_row* __restrict__ table,
                                                            const uint32_t* __restrict__ bits, long t_stride, int nT, int slot,
                                                            const int32_t* __restrict__ state, int repeat_first) {
    constexpr int N = Vec<T>::N;
    const pdmk_mask_row r = table[blockIdx.x];
    if (r.O <= 0 || r.F <= 0 || r.ld < r.F || r.dst_off < 0 || r.src_off < 0 || r.bits_off < 0) return;
    int s = slot;
    if (state) {
        s = state[0];
        if (repeat_first && s > 0) --s;                       // PNDM: calls 0 and 1 are the same timestep
    }
    const uint32_t* b = (bits && s >= 0 && s < nT) ? bits + (long)s * t_stride + r.bits_off : nullptr;
    const int rw = (r.F + 31) >> 5;
    T* d = dst + r.dst_off;
    const T* p = src + r.src_off;
    if (!((r.F | r.ld | r.dst_off | r.src_off) & (N - 1))) {
        const int cpr = r.F / N;                              // chunks per row
        const int n = r.O * cpr;
        for (int i = threadIdx.x; i < n; i += NT) {
            const int o = i / cpr, f0 = (i - o * cpr) * N;
            typename Vec<T>::raw v = Vec<T>::load_raw(p + (long)o * r.ld + f0);
            if (b) {
                const uint32_t m = b[(long)o * rw + (f0 >> 5)] >> (f0 & 31);       // N divides 32: a chunk is inside one word
#pragma unroll
                for (int e = 0; e < N; ++e) v[e] = ((m >> e) & 1u) ? (T)0.f : v[e];
            }
            *reinterpret_cast<typename Vec<T>::raw*>(d + (long)o * r.ld + f0) = v;
        }
    } else {
        const int n = r.O * r.F;
        for (int i = threadIdx.x; i < n; i += NT) {
            const int o = i / r.F, f = i - o * r.F;
            T v = p[(long)o * r.ld + f];
            if (b && ((b[(long)o * rw + (f >> 5)] >> (f & 31)) & 1u)) v = (T)0.f;
            d[(long)o * r.ld + f] = v;
        }
    }
}

template <typename T>
int masked_weights_t(void* dst, const void* src, const pdmk_mask_row* table, int nrows, const uint32_t* bits, long t_stride, int nT,
                     int slot, const int32_t* state, int repeat_first, hipStream_t st) {
    hipLaunchKernelGGL(masked_weights_kernel<T>, dim3(nrows), dim3(NT), 0, st, (T*)dst, (const T*)src, table, bits, t_stride, nT,
                       slot, state, repeat_first);
    PDMK_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int64_t pdmk_rownorm_colsq_workspace_elems(int M, int F) {
    if (M < 1 || F < 8) return 0;
    const int rpb = colsq_rows_per_block(M, F);
    const int nrb = (M + rpb - 1) / rpb;
    return ((int64_t)M + 63) / 64 * 64 + (int64_t)nrb * F;
}

extern "C" int pdmk_rownorm_colsq(const void* x, int dtype, int M, int F, int ld, float* acc, float* ws, int64_t ws_elems,
                                  pdmk_stream s) {
    if (!x || !acc || !ws || M < 1 || F < 8 || F % 8 || ld < F || ld % 8 || ((uintptr_t)x & 15) || ((uintptr_t)ws & 15) ||
        ws_elems < pdmk_rownorm_colsq_workspace_elems(M, F))
        return -1;
    PDMK_DISPATCH(dtype, rownorm_colsq_t, x, M, F, ld, acc, ws, (hipStream_t)s);
}

extern "C" int pdmk_wanda_count(const void* w, int dtype, int O, int F, int ldw, const float* n_base, const float* n_target, int T,
                                int k, int32_t* count, pdmk_stream s) {
    if (!w || !n_base || !n_target || !count || O < 1 || F < 1 || ldw < F || T < 1 || k < 0) return -1;
    if (F > PDMK_WANDA_MAX_F) return -2;
    if (k == 0) return 0;                                      // nothing is selected
    PDMK_DISPATCH(dtype, wanda_count_t, w, O, F, ldw, n_base, n_target, T, k, count, (hipStream_t)s);
}

extern "C" int pdmk_wanda_select(const void* w, int dtype, int O, int F, int ldw, const float* n_base, const float* n_target, int T,
                                 int k, uint32_t* bits, int64_t t_stride, pdmk_stream s) {
    if (!w || !n_base || !n_target || !bits || O < 1 || F < 1 || ldw < F || T < 1 || k < 0 || ((uintptr_t)bits & 3)) return -1;
    if (F > PDMK_WANDA_MAX_F) return -2;
    if (t_stride < (int64_t)O * ((F + 31) / 32)) return -1;
    PDMK_DISPATCH(dtype, wanda_select_t, w, O, F, ldw, n_base, n_target, T, k, bits, (long)t_stride, (hipStream_t)s);
}

extern "C" int pdmk_masked_weights(void* dst, const void* src, int dtype, const pdmk_mask_row* table, int nrows,
                                   const uint32_t* bits, int64_t t_stride, int T, int slot, const int32_t* state, int repeat_first,
                                   pdmk_stream s) {
    if (!dst || !src || !table || nrows < 1 || T < 0 || t_stride < 0 || (((uintptr_t)dst | (uintptr_t)src) & 15) ||
        ((uintptr_t)table & 7) || ((uintptr_t)bits & 3) || ((uintptr_t)state & 3))
        return -1;
    PDMK_DISPATCH(dtype, masked_weights_t, dst, src, table, nrows, bits, (long)t_stride, T, slot, state, repeat_first,
                  (hipStream_t)s);
}

extern "C" int pdmk_wanda_apply(void* w, int dtype, int O, int F, int ldw, const int32_t* count, float threshold, pdmk_stream s) {
    if (!w || !count || O < 1 || F < 1 || ldw < F) return -1;
    PDMK_DISPATCH(dtype, wanda_apply_t, w, O, F, ldw, count, threshold, (hipStream_t)s);
}
