// GroupNorm(+SiLU) and LayerNorm, forward and backward, NHWC / token-major, HBM-bandwidth kernels.
// All loads/stores are 16-byte chunks along the channel dim (rows are read fully coalesced); statistics are fp32
// per thread, fp32 LDS atomics per block, then double atomics across blocks so that E[x^2]-mean^2 is formed in double.
#include <initializer_list>
#include <type_traits>

#include "common.h"
#include "vec.h"

namespace {

constexpr int NT = 256;
constexpr int MAXS = 3;   // chunk slots per thread: C/chunk <= 3*256

// Second stage of the per-channel parameter-gradient reductions: part[b][2][n] (one slab per first-stage block, plain
// stores) -> out0[n] += sum_b part[b][0][:], out1[n] += sum_b part[b][1][:].  Many blocks hammering the same few hundred
// addresses with float atomics serialise at the memory side (measured 130 us for a 10 us LayerNorm backward); two
// stages with at most 8 adds per address do not.
__global__ void reduce_partials_kernel(const float* __restrict__ part, int nblk, int n, float* __restrict__ out0,
                                       float* __restrict__ out1) {
    const int j = blockIdx.x * NT + threadIdx.x;
    if (j >= 2 * n) return;
    const int per = (nblk + gridDim.y - 1) / gridDim.y;
    const int b0 = blockIdx.y * per, b1 = min(nblk, b0 + per);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int b = b0;
    for (; b + 3 < b1; b += 4) {
        s0 += part[(long)b * 2 * n + j];
        s1 += part[(long)(b + 1) * 2 * n + j];
        s2 += part[(long)(b + 2) * 2 * n + j];
        s3 += part[(long)(b + 3) * 2 * n + j];
    }
    for (; b < b1; ++b) s0 += part[(long)b * 2 * n + j];
    const float s = (s0 + s1) + (s2 + s3);
    if (b1 > b0) unsafeAtomicAdd(j < n ? out0 + j : out1 + (j - n), s);
}
inline void launch_reduce_partials(const float* part, int nblk, int n, float* out0, float* out1, hipStream_t st) {
    if (!out0 && !out1) return;          // deferred: the caller reduces this slab later with pdmk_reduce_partials_group
    const int slices = nblk >= 256 ? 8 : (nblk >= 32 ? 4 : 1);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((2 * n + NT - 1) / NT, slices), dim3(NT), 0, st, part, nblk, n, out0,
                       out1);
}

// The same second stage for up to PDMK_PARTIAL_GROUP_MAX slabs in ONE launch (the per-layer launches are ~7 us each for
// ~1 us of traffic, and a training step has ~110 of them): blockIdx.y = item * 8 + slice.
struct PartialGroup {
    pdmk_partial_item it[PDMK_PARTIAL_GROUP_MAX];
};
__global__ void reduce_partials_group_kernel(PartialGroup gr) {
    const pdmk_partial_item it = gr.it[blockIdx.y >> 3];
    const int slice = blockIdx.y & 7, n = it.n, nblk = it.nblk;
    const int j = blockIdx.x * NT + threadIdx.x;
    if (j >= 2 * n) return;
    const int per = (nblk + 7) / 8;
    const int b0 = slice * per, b1 = min(nblk, b0 + per);
    const float* part = it.part;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int b = b0;
    for (; b + 3 < b1; b += 4) {
        s0 += part[(long)b * 2 * n + j];
        s1 += part[(long)(b + 1) * 2 * n + j];
        s2 += part[(long)(b + 2) * 2 * n + j];
        s3 += part[(long)(b + 3) * 2 * n + j];
    }
    for (; b < b1; ++b) s0 += part[(long)b * 2 * n + j];
    const float s = (s0 + s1) + (s2 + s3);
    if (b1 > b0) unsafeAtomicAdd(j < n ? it.out0 + j : it.out1 + (j - n), s);
}

// ------------------------------------------------------------------------------------------------ GroupNorm
// Thread map: a block sweeps rows [r0, r1) of one image; thread (cb, ro) owns 16-byte chunk cb (+ tpr*slot) of row
// ro (+ rif*k).  UNR rows are loaded per iteration before any of them is used (UNR independent 16-byte loads in flight
// per thread: these kernels are pure HBM streams, and a CU needs tens of KiB in flight to reach HBM bandwidth).
// Reductions never use atomics: per-block partials go to a slab with plain stores and the consumer kernel's prologue
// adds the (<= 64) slabs of its image in double (E[x^2] - mean^2 is formed in double).
struct GnMap2 {
    int tpr, rif;   // threads per row (= chunks per row, capped at 256), rows in flight
};
__host__ __device__ inline GnMap2 gn_map2(int nchunks) {
    const int tpr = nchunks < NT ? nchunks : NT;
    return GnMap2{tpr, NT / tpr};
}
constexpr int GN_MAXC = MAXS * NT * 8;   // channel capacity of the LDS reduction image (bf16 chunks)
constexpr int GN_MAXBLK = 64;            // stats blocks per image

// One thread's place in the map above, and the shape it was built from.
struct GnThread {
    int C, HW, nchunks, cr;   // cr = G * gs: the normalised channels (channels from cr on are padding)
    GnMap2 mp;
    int cb, ro, b, r0, r1;
    bool active;              // ro < rif (a tpr that does not divide 256 leaves threads over)
    __device__ __forceinline__ int chunk(int sl) const { return cb + mp.tpr * sl; }
    __device__ __forceinline__ long row(int rr) const { return (long)b * HW + rr; }
};
template <int V>
__device__ __forceinline__ GnThread gn_thread(int C, int HW, int rows_per_blk, int G, int gs) {
    GnThread t;
    t.C = C, t.HW = HW, t.nchunks = C / V;
    t.mp = gn_map2(t.nchunks);
    const int tid = threadIdx.x;
    t.cb = tid % t.mp.tpr, t.ro = tid / t.mp.tpr;
    t.b = blockIdx.y;
    t.r0 = blockIdx.x * rows_per_blk, t.r1 = min(HW, t.r0 + rows_per_blk);
    t.cr = G * gs;
    t.active = t.ro < t.mp.rif;
    return t;
}
__device__ __forceinline__ bool gn_aligned16(const float* gamma, const float* beta) {
    return ((reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta)) & 15) == 0;
}

// gamma / beta of chunk slot sl: 16-byte loads where the whole chunk lies inside the normalised channels and both pointers are
// 16-byte aligned (vec_gb), element by element (0 for padding channels and for chunks this thread does not own) otherwise
template <int V>
__device__ __forceinline__ void gn_load_gb(const GnThread& t, int sl, const float* gamma, const float* beta, bool vec_gb,
                                           float* gm, float* bt) {
    const int c = t.chunk(sl);
    if (t.active && c < t.nchunks && c * V + V <= t.cr && vec_gb) {
#pragma unroll
        for (int e = 0; e < V; e += 4) {
            const float4 g4 = *reinterpret_cast<const float4*>(gamma + c * V + e), b4 = *reinterpret_cast<const float4*>(beta + c * V + e);
            gm[e] = g4.x; gm[e + 1] = g4.y; gm[e + 2] = g4.z; gm[e + 3] = g4.w;
            bt[e] = b4.x; bt[e + 1] = b4.y; bt[e + 2] = b4.z; bt[e + 3] = b4.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int ch = c * V + e;
            const bool ok = t.active && c < t.nchunks && ch < t.cr;
            gm[e] = ok ? gamma[ch] : 0.f;
            bt[e] = ok ? beta[ch] : 0.f;
        }
    }
}

// The row sweeps of one thread over NSRC tensors that are streamed in step (x, or x and dy): a register ping-pong, pre -> cur.
// preload(sl) issues slot sl's first sweep; a kernel calls it next to gn_load_gb, in front of everything that waits for the
// statistics (gn_apply_kernel says why).  run() then hands every valid (slot, chunk, row, raw 16-byte values of that cell) to
// `body`, with the next sweep's loads issued before this sweep's arithmetic.  Only active threads call run().
template <typename T, int UNR, int SLOTS, int NSRC>
struct GnSweep {
    typedef typename Vec<T>::raw Raw;
    static constexpr int V = Vec<T>::N;
    const T* src[NSRC];
    int ld[NSRC];
    Raw pre[SLOTS][UNR][NSRC];
    __device__ __forceinline__ GnSweep(const T* s0, int ld0, const T* s1 = nullptr, int ld1 = 0) {
        src[0] = s0, ld[0] = ld0;
        if (NSRC > 1) src[NSRC - 1] = s1, ld[NSRC - 1] = ld1;
    }
    __device__ __forceinline__ void load(const GnThread& t, int sl, int u, int c, int rr) {
#pragma unroll
        for (int k = 0; k < NSRC; ++k) pre[sl][u][k] = Vec<T>::load_raw(src[k] + t.row(rr) * ld[k] + c * V);
    }
    __device__ __forceinline__ void preload(const GnThread& t, int sl) {
        const int c = t.chunk(sl);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int rr = t.r0 + t.ro + u * t.mp.rif;
            if (t.active && c < t.nchunks && rr < t.r1) load(t, sl, u, c, rr);
        }
    }
    template <typename F>
    __device__ __forceinline__ void run(const GnThread& t, F&& body) {
        const int step = t.mp.rif * UNR;
        for (int r = t.r0 + t.ro; r < t.r1; r += step) {
            Raw cur[SLOTS][UNR][NSRC];
#pragma unroll
            for (int sl = 0; sl < SLOTS; ++sl) {
                const int c = t.chunk(sl);
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
#pragma unroll
                    for (int k = 0; k < NSRC; ++k) cur[sl][u][k] = pre[sl][u][k];
                    const int rn = r + step + u * t.mp.rif;           // the next sweep's loads go out before this sweep's arithmetic
                    if (c < t.nchunks && rn < t.r1) load(t, sl, u, c, rn);
                }
            }
#pragma unroll
            for (int sl = 0; sl < SLOTS; ++sl) {
                const int c = t.chunk(sl);
                if (c < t.nchunks) {
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const int rr = r + u * t.mp.rif;
                        if (rr < t.r1) body(sl, c, rr, cur[sl][u]);
                    }
                }
            }
        }
    }
};

// Per-group values expanded to the V channels of chunk slot sl: one division per chunk; the group index then steps with the
// channel.  body(e, g, ok): element e belongs to group g; ok = a normalised channel of a chunk this thread owns
template <int V, typename F>
__device__ __forceinline__ void gn_for_channels(const GnThread& t, int sl, int gs, F&& body) {
    const int c = t.chunk(sl);
    int g = (c * V) / gs, rem = c * V - g * gs;
#pragma unroll
    for (int e = 0; e < V; ++e) {
        body(e, g, c < t.nchunks && c * V + e < t.cr);
        if (++rem == gs) { rem = 0; ++g; }
    }
}

// the per-thread sums of an active thread -> the [rif][C] LDS images red[0], red[1]
template <int V, int SLOTS, int N>
__device__ __forceinline__ void gn_red_store(const GnThread& t, float (&red)[2][N], const float (&s0)[SLOTS][V],
                                             const float (&s1)[SLOTS][V]) {
    if (!t.active) return;
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        const int c = t.chunk(sl);
        if (c < t.nchunks) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                red[0][t.ro * t.C + c * V + e] = s0[sl][e];
                red[1][t.ro * t.C + c * V + e] = s1[sl][e];
            }
        }
    }
}

// 256 partials, [quarter][64], of at most 64 sums -> the sum of thread tid's four, quarters 0 + 1 and 2 + 3 first
template <typename F>
__device__ __forceinline__ F gn_fold4(const F* q, int tid) {
    return (q[tid] + q[tid + 64]) + (q[tid + 128] + q[tid + 192]);
}

// 256 threads: (group g = tid % 64, quarter = tid / 64) -> partial over a quarter of group g's `cells` cells of the two images
// (cell i of group g is red[.][at(g, i)]), the four quarters folded, group g's (sum0, sum1) stored to slab[2 * g].  The images
// must be complete (a barrier behind their last write); they are overwritten.
template <int N, typename At>
__device__ __forceinline__ void gn_group_sums_store(float (&red)[2][N], int G, int cells, At&& at, float* slab) {
    const int tid = threadIdx.x, g = tid & 63, qt = tid >> 6;
    float ps = 0.f, pq = 0.f;
    if (g < G)
        for (int i = qt; i < cells; i += 4) {
            const int j = at(g, i);
            ps += red[0][j];
            pq += red[1][j];
        }
    __syncthreads();
    red[0][tid] = ps;
    red[1][tid] = pq;
    __syncthreads();
    if (tid < G) {
        slab[2 * tid] = gn_fold4(red[0], tid);
        slab[2 * tid + 1] = gn_fold4(red[1], tid);
    }
}

// sums the nblk per-block (sum0, sum1) slabs of image b into LDS out0[g], out1[g] (double); all 256 threads take part
__device__ __forceinline__ void gn_sum_slabs(const float* __restrict__ part, int b, int nblk, int G, double* out0,
                                             double* out1, double (*scr)[NT]) {
    const int tid = threadIdx.x, g = tid & 63, qt = tid >> 6;
    double a0 = 0.0, a1 = 0.0;
    if (g < G)
        for (int k = qt; k < nblk; k += 4) {
            const float* slab = part + (((long)b * nblk + k) * G + g) * 2;
            a0 += (double)slab[0];
            a1 += (double)slab[1];
        }
    scr[0][tid] = a0;
    scr[1][tid] = a1;
    __syncthreads();
    if (tid < G) {
        out0[tid] = gn_fold4(scr[0], tid);
        out1[tid] = gn_fold4(scr[1], tid);
    }
    __syncthreads();
}

// (its row loop loads UNR rows and then consumes them, with no ping-pong, so it is written out here and is not a GnSweep)
template <typename T, int UNR, int SLOTS>
__global__ __launch_bounds__(NT) void gn_stats_kernel(const T* __restrict__ x, float* __restrict__ part, int HW, int C,
                                                      int ldx, int G, int gs, int rows_per_blk) {
    constexpr int V = Vec<T>::N;
    const GnThread t = gn_thread<V>(C, HW, rows_per_blk, G, gs);
    float s[SLOTS][V], q[SLOTS][V];
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl)
#pragma unroll
        for (int e = 0; e < V; ++e) s[sl][e] = q[sl][e] = 0.f;
    if (t.active) {
        for (int r = t.r0 + t.ro; r < t.r1; r += t.mp.rif * UNR) {
#pragma unroll
            for (int sl = 0; sl < SLOTS; ++sl) {
                const int c = t.chunk(sl);
                if (c < t.nchunks) {
                    float f[UNR][V];
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const int rr = r + u * t.mp.rif;
                        if (rr < t.r1) Vec<T>::load(x + t.row(rr) * ldx + c * V, f[u]);
                        else {
#pragma unroll
                            for (int e = 0; e < V; ++e) f[u][e] = 0.f;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < UNR; ++u)
#pragma unroll
                        for (int e = 0; e < V; ++e) { s[sl][e] += f[u][e]; q[sl][e] += f[u][e] * f[u][e]; }
                }
            }
        }
    }
    __shared__ float red[2][GN_MAXC / 8 * V];
    gn_red_store<V, SLOTS>(t, red, s, q);
    __syncthreads();
    gn_group_sums_store(red, G, t.mp.rif * gs, [&](int g, int i) { const int rr = i / gs; return rr * C + g * gs + (i - rr * gs); },
                        part + ((long)t.b * gridDim.x + blockIdx.x) * G * 2);
}

template <typename T, int UNR, int SLOTS>
__global__ __launch_bounds__(NT) void gn_apply_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ part, int nblk,
                                                      float* __restrict__ stats, int HW,
                                                      int C, int ldx, int ldy, int G, int gs, float eps, int silu,
                                                      int rows_per_blk, int cs_ld = 0) {
    constexpr int V = Vec<T>::N;
    const GnThread t = gn_thread<V>(C, HW, rows_per_blk, G, gs);
    const int tid = threadIdx.x, b = t.b;
    __shared__ double scr[2][NT], d0[64], d1[64];
    __shared__ float lm[64], lr[64];
    // Everything that does not depend on the statistics is issued FIRST - this thread's gamma / beta chunks and its first sweep of
    // rows - so that those loads are in flight while the block works out mean / rstd (a chain of an L2 read, an LDS reduction and
    // a double-precision sqrt: 3-4 us per block, which every block of the grid pays at the same time; with the loads behind it the
    // kernel streamed at 2.5 TB/s where a plain copy of the same tensor reaches 6.4, tools/gn_bench.py).
    const bool vec_gb = gn_aligned16(gamma, beta);
    // (the statistics' own loads are the very first: loads return in issue order, so behind the row sweep they would wait for it)
    long long l0 = 0, h0 = 0, l1 = 0, h1 = 0;
    int cs_bad = 0;
    if (nblk < 0 && (tid >> 2) < G) {
        // epilogue statistics (pdmk_gemm_args.colstat): `part` = this tensor's first column of the [B][4][cs_ld] per-(image, column)
        // fixed-point sums (two limbs each); group g = its gs columns.  4 threads per group (G <= 64): thread (g, p) adds the limbs of
        // columns p, p + 4, ... in registers, the partners are folded with two shuffles below.  Exact integer sums, no atomics
        // (LDS atomics here put 40 same-address adds of one group into one wave instruction: 8 us per block)
        const long long* cg = reinterpret_cast<const long long*>(part) + (long)b * 4 * cs_ld + (tid >> 2) * gs;
#pragma unroll 4
        for (int j = tid & 3; j < gs; j += 4) {
            const long long q3 = cg[3 * cs_ld + j];
            l0 += cg[j];
            h0 += cg[cs_ld + j];
            l1 += cg[2 * cs_ld + j];
            h1 += cs_strip(q3);
            cs_bad |= cs_flagged(q3) ? 1 : 0;                   // a producer's partial sum was NaN / inf (common.h cs_add)
        }
    }
    float gmv[SLOTS][V], btv[SLOTS][V];
    GnSweep<T, UNR, SLOTS, 1> sweep(x, ldx);
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        gn_load_gb<V>(t, sl, gamma, beta, vec_gb, gmv[sl], btv[sl]);
        sweep.preload(t, sl);
    }
    if (nblk < 0) {
        const int g = tid >> 2, pth = tid & 3;
#pragma unroll
        for (int m = 1; m < 4; m <<= 1) {
            l0 += __shfl_xor(l0, m, 64);
            h0 += __shfl_xor(h0, m, 64);
            l1 += __shfl_xor(l1, m, 64);
            h1 += __shfl_xor(h1, m, 64);
        }
        cs_bad |= __shfl_xor(cs_bad, 1, 64);
        cs_bad |= __shfl_xor(cs_bad, 2, 64);
        if (g < G && pth == 0) {                                 // non-finite input -> non-finite statistics, as a statistics pass gives
            d0[g] = cs_bad ? __builtin_nan("") : cs_value(l0, h0);
            d1[g] = cs_bad ? __builtin_nan("") : cs_value(l1, h1);
        }
        __syncthreads();
    } else {
        gn_sum_slabs(part, b, nblk, G, d0, d1, scr);
    }
    if (tid < G) {
        // (double where the cancellation is: E[x^2] - mean^2 - INCLUDING 1 / n, whose error multiplies mean^2: the fp32 v_rcp seeds
        // it and two Newton steps in double bring it to ~1e-16 relative (a 6e-8 inv_n would leave 6e-8 * mean^2 / var in the
        // variance of a channel group with |mean| >> std - ADVICE r3).  Only the square root stays fp32 - v_rsq refined once: the
        // fp64 div + sqrt this replaces were ~1 us of every block's prologue, two double fma pairs are not)
        const double nd = (double)HW * (double)gs;
        double inv_n = (double)__frcp_rn((float)nd);
        inv_n = inv_n * (2.0 - nd * inv_n);
        inv_n = inv_n * (2.0 - nd * inv_n);
        const double mean = d0[tid] * inv_n;
        double var = d1[tid] * inv_n - mean * mean;
        if (var < 0) var = 0;
        const float ve = (float)(var + (double)eps);
        float rstd = __frsqrt_rn(ve);
        rstd = rstd * (1.5f - 0.5f * ve * rstd * rstd);
        lm[tid] = (float)mean;
        lr[tid] = rstd;
        if (blockIdx.x == 0) {
            stats[((long)b * G + tid) * 2] = (float)mean;
            stats[((long)b * G + tid) * 2 + 1] = rstd;
        }
    }
    __syncthreads();
    if (!t.active) return;
    float sc[SLOTS][V], sh[SLOTS][V];   // y = x*sc + sh  (pad channels: 0)
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl)
        gn_for_channels<V>(t, sl, gs, [&](int e, int g, bool ok) {
            sc[sl][e] = sh[sl][e] = 0.f;
            if (ok) {
                const float a = lr[g] * gmv[sl][e];
                sc[sl][e] = a;
                sh[sl][e] = btv[sl][e] - lm[g] * a;
            }
        });
    sweep.run(t, [&](int sl, int c, int rr, const auto& raw) {
        float f[V];
        Vec<T>::unpack(raw[0], f);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float z = f[e] * sc[sl][e] + sh[sl][e];
            f[e] = silu ? silu_f(z) : z;
        }
        Vec<T>::store(y + t.row(rr) * ldy + c * V, f);
    });
}

// backward pass 1: per (b,g) s1 = sum gamma*dz, s2 = sum gamma*dz*xhat (slab `gpart`); per channel dgamma += sum
// dz*xhat, dbeta += sum dz (slab `part`, second stage reduce_partials_kernel)
template <typename T, int UNR, int SLOTS>
__global__ __launch_bounds__(NT) void gn_bwd_stats_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          const float* __restrict__ stats, float* __restrict__ part,
                                                          float* __restrict__ gpart, int HW,
                                                          int C, int ldx, int lddy, int G, int gs, int silu,
                                                          int rows_per_blk) {
    constexpr int V = Vec<T>::N;
    const GnThread t = gn_thread<V>(C, HW, rows_per_blk, G, gs);
    const int tid = threadIdx.x, b = t.b, cr = t.cr;
    float a1[SLOTS][V], a2[SLOTS][V], mean[SLOTS][V], rstd[SLOTS][V], gm[SLOTS][V], bt[SLOTS][V];
    // as gn_apply_kernel: 16-byte gamma / beta loads and the first sweep of rows go out first, (mean, rstd) through LDS (one
    // coalesced load per group instead of two scalar loads and a division per channel), then a register ping-pong over the sweeps
    __shared__ float sm[64], sr[64];
    const bool vec_gb = gn_aligned16(gamma, beta);
    GnSweep<T, UNR, SLOTS, 2> sweep(x, ldx, dy, lddy);
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        gn_load_gb<V>(t, sl, gamma, beta, vec_gb, gm[sl], bt[sl]);
        sweep.preload(t, sl);
    }
    if (tid < G) {
        sm[tid] = stats[((long)b * G + tid) * 2];
        sr[tid] = stats[((long)b * G + tid) * 2 + 1];
    }
    __syncthreads();
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl)
        gn_for_channels<V>(t, sl, gs, [&](int e, int g, bool ok) {
            a1[sl][e] = a2[sl][e] = 0.f;
            mean[sl][e] = rstd[sl][e] = 0.f;
            if (ok) {
                mean[sl][e] = sm[g];
                rstd[sl][e] = sr[g];
            } else {
                gm[sl][e] = bt[sl][e] = 0.f;
            }
        });
    if (t.active)
        sweep.run(t, [&](int sl, int c, int rr, const auto& raw) {
            float f[V], d[V];
            Vec<T>::unpack(raw[0], f);
            Vec<T>::unpack(raw[1], d);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float xh = (f[e] - mean[sl][e]) * rstd[sl][e];
                float dz = d[e];
                if (silu) dz *= silu_grad_f(xh * gm[sl][e] + bt[sl][e]);
                a1[sl][e] += dz;
                a2[sl][e] += dz * xh;
            }
        });
    __shared__ float red[2][GN_MAXC / 8 * V];
    gn_red_store<V, SLOTS>(t, red, a1, a2);
    __syncthreads();
    // per-channel sums over the rows in flight -> row 0 of the image (+ the dgamma/dbeta slab of this block)
    float* slab = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2 * cr;                 // [dgamma | dbeta]
    for (int ch = tid; ch < cr; ch += NT) {
        float t1 = 0.f, t2 = 0.f;
        for (int rr = 0; rr < t.mp.rif; ++rr) { t1 += red[0][rr * C + ch]; t2 += red[1][rr * C + ch]; }
        slab[ch] = t2;
        slab[cr + ch] = t1;
        const float gmc = gamma[ch];
        red[0][ch] = gmc * t1;      // only row 0 is read below; rows >= 1 of other channels are not touched by this thread
        red[1][ch] = gmc * t2;
    }
    __syncthreads();
    gn_group_sums_store(red, G, gs, [&](int g, int i) { return g * gs + i; }, gpart + ((long)b * gridDim.x + blockIdx.x) * G * 2);
}

template <typename T, int UNR, int SLOTS>
__global__ __launch_bounds__(NT) void gn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                          T* __restrict__ dx, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          const float* __restrict__ stats,
                                                          const float* __restrict__ gpart, int nblk, int HW, int C,
                                                          int ldx, int lddy, int lddx, int G, int gs, int silu,
                                                          int accumulate, int rows_per_blk, const T* __restrict__ add,
                                                          int ldadd) {
    constexpr int V = Vec<T>::N;
    const GnThread t = gn_thread<V>(C, HW, rows_per_blk, G, gs);
    const int tid = threadIdx.x, b = t.b;
    __shared__ double scr[2][NT], d0[64], d1[64];
    __shared__ float sm[64], sr[64];
    // as gn_apply_kernel: what does not depend on the group sums goes out first (gamma / beta chunks, the (mean, rstd) pairs, the
    // first sweep of x / dy rows), so that it is in flight while the block adds up the slabs.
    // The sweep is written out here and is not a GnSweep: through the helper the two-slot bf16 instance came out with another
    // schedule and 0.3 - 0.6 us slower at 8 x 256 x 2560 (profiles/gn_refactor_bench.txt); written out, the two- and three-slot
    // instances are instruction for instruction what they were before the helpers.
    typedef typename Vec<T>::raw Raw;
    const bool vec_gb = gn_aligned16(gamma, beta);
    float gm[SLOTS][V], bt[SLOTS][V];
    Raw px[SLOTS][UNR], pd[SLOTS][UNR];
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        gn_load_gb<V>(t, sl, gamma, beta, vec_gb, gm[sl], bt[sl]);
        const int c = t.chunk(sl);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int rr = t.r0 + t.ro + u * t.mp.rif;
            if (t.active && c < t.nchunks && rr < t.r1) {
                px[sl][u] = Vec<T>::load_raw(x + t.row(rr) * ldx + c * V);
                pd[sl][u] = Vec<T>::load_raw(dy + t.row(rr) * lddy + c * V);
            }
        }
    }
    if (tid < G) {
        sm[tid] = stats[((long)b * G + tid) * 2];
        sr[tid] = stats[((long)b * G + tid) * 2 + 1];
    }
    gn_sum_slabs(gpart, b, nblk, G, d0, d1, scr);          // (ends with a barrier: sm / sr are visible too)
    if (!t.active) return;
    const float invn = 1.0f / ((float)HW * (float)gs);
    float mean[SLOTS][V], rstd[SLOTS][V], c1[SLOTS][V], c2[SLOTS][V];
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl)
        gn_for_channels<V>(t, sl, gs, [&](int e, int g, bool ok) {
            mean[sl][e] = rstd[sl][e] = c1[sl][e] = c2[sl][e] = 0.f;
            if (ok) {
                mean[sl][e] = sm[g];
                rstd[sl][e] = sr[g];
                c1[sl][e] = (float)d0[g] * invn;
                c2[sl][e] = (float)d1[g] * invn;
            }
        });
    const int step = t.mp.rif * UNR;
    for (int r = t.r0 + t.ro; r < t.r1; r += step) {
        Raw cx[SLOTS][UNR], cd[SLOTS][UNR];
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            const int c = t.chunk(sl);
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                cx[sl][u] = px[sl][u];
                cd[sl][u] = pd[sl][u];
                const int rn = r + step + u * t.mp.rif;           // as GnSweep::run: the next sweep's loads first
                if (c < t.nchunks && rn < t.r1) {
                    px[sl][u] = Vec<T>::load_raw(x + t.row(rn) * ldx + c * V);
                    pd[sl][u] = Vec<T>::load_raw(dy + t.row(rn) * lddy + c * V);
                }
            }
        }
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            const int c = t.chunk(sl);
            if (c < t.nchunks) {
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int rr = r + u * t.mp.rif;
                    if (rr < t.r1) {
                        float f[V], d[V], o[V], a2[V];
                        Vec<T>::unpack(cx[sl][u], f);
                        Vec<T>::unpack(cd[sl][u], d);
                        if (accumulate) Vec<T>::load(dx + t.row(rr) * lddx + c * V, o);
                        if (add) Vec<T>::load(add + t.row(rr) * ldadd + c * V, a2);
#pragma unroll
                        for (int e = 0; e < V; ++e) {
                            const float xh = (f[e] - mean[sl][e]) * rstd[sl][e];
                            float dz = d[e];
                            if (silu) dz *= silu_grad_f(xh * gm[sl][e] + bt[sl][e]);
                            float v = rstd[sl][e] * (gm[sl][e] * dz - c1[sl][e] - xh * c2[sl][e]);
                            if (add) v += a2[e];           // a second finished gradient of x (residual fan-in) folded in
                            o[e] = accumulate ? o[e] + v : v;
                        }
                        Vec<T>::store(dx + t.row(rr) * lddx + c * V, o);
                    }
                }
            }
        }
    }
}

// rows per block for ~target_blocks blocks chip-wide (at most max_blk per image, at least one sweep of rows per block)
inline int gn_rows_per_blk(int B, int HW, int sweep, int target_blocks, int max_blk) {
    int nb = (target_blocks + B - 1) / B;
    nb = max(1, min(min(nb, max_blk), HW / max(1, sweep)));
    int rpb = (HW + nb - 1) / nb;
    // whole sweeps (rows in flight x unroll) per block: a ragged last sweep runs with a fraction of the threads
    rpb = (rpb + sweep - 1) / sweep * sweep;
    return rpb;
}

// The four launches: rows of one sweep / rif (the kernel's UNR), block target chip-wide, blocks per image at most.  The UNR
// template arguments, the sweep given to gn_rows_per_blk and the grid all come from here.
struct GnLaunch {
    int unr, target_blocks, max_blk;
};
constexpr GnLaunch GN_FWD_STATS{8, 512, GN_MAXBLK}, GN_FWD_APPLY{4, 1024, 1 << 20}, GN_BWD_STATS{4, 512, GN_MAXBLK},
    GN_BWD_APPLY{2, 1024, 1 << 20};
struct GnGrid {
    int rpb;     // rows per block
    dim3 grid;   // (blocks per image, B)
};
inline GnGrid gn_grid(const GnLaunch& l, int B, int HW, int nchunks) {
    const int rpb = gn_rows_per_blk(B, HW, gn_map2(nchunks).rif * l.unr, l.target_blocks, l.max_blk);
    return GnGrid{rpb, dim3((HW + rpb - 1) / rpb, B)};
}

// what every launcher refuses; red_image: the kernels keep their sums in the `red` LDS image (GN_MAXC channels of bf16 chunks)
template <int V>
inline bool gn_shape_ok(int C, int G, int gs, std::initializer_list<int> lds, bool red_image) {
    for (int ld : lds)
        if (ld % V) return false;
    return !(C % V || G > 64 || G * gs > C || C / V > MAXS * NT || (red_image && C > GN_MAXC / 8 * V));
}

// f(std::integral_constant<int, SLOTS>) for the chunk slots a thread needs
template <typename F>
inline void gn_dispatch_slots(int nchunks, F&& f) {
    const int slots = (nchunks + NT - 1) / NT;
    if (slots == 1) f(std::integral_constant<int, 1>());
    else if (slots == 2) f(std::integral_constant<int, 2>());
    else f(std::integral_constant<int, 3>());
}

template <typename T>
int gn_fwd(const void* x, void* y, const float* gamma, const float* beta, float* stats, double* ws, int B, int HW,
           int C, int ldx, int ldy, int G, int gs, float eps, int silu, hipStream_t st) {
    constexpr int V = Vec<T>::N;
    if (!gn_shape_ok<V>(C, G, gs, {ldx, ldy}, true)) return -1;
    float* part = reinterpret_cast<float*>(ws);                     // [B][nblk][G][2] floats <= B*G*64 doubles
    const GnGrid gst = gn_grid(GN_FWD_STATS, B, HW, C / V), gap = gn_grid(GN_FWD_APPLY, B, HW, C / V);
    gn_dispatch_slots(C / V, [&](auto slots) {
        constexpr int S = decltype(slots)::value;
        hipLaunchKernelGGL((gn_stats_kernel<T, GN_FWD_STATS.unr, S>), gst.grid, dim3(NT), 0, st, (const T*)x, part, HW, C, ldx, G,
                           gs, gst.rpb);
        hipLaunchKernelGGL((gn_apply_kernel<T, GN_FWD_APPLY.unr, S>), gap.grid, dim3(NT), 0, st, (const T*)x, (T*)y, gamma, beta,
                           part, (int)gst.grid.x, stats, HW, C, ldx, ldy, G, gs, eps, silu, gap.rpb);
    });
    PDMK_CHECK_LAUNCH();
    return 0;
}

// statistics from the producing GEMM's epilogue (pdmk_gemm_args.colstat): the apply launch alone, nblk = -1
template <typename T>
int gn_apply_colstat(const void* x, void* y, const float* gamma, const float* beta, float* stats, const int64_t* colstat, int cs_ld,
                     int B, int HW, int C, int ldx, int ldy, int G, int gs, float eps, int silu, hipStream_t st) {
    constexpr int V = Vec<T>::N;
    if (!gn_shape_ok<V>(C, G, gs, {ldx, ldy}, false)) return -1;
    const GnGrid gap = gn_grid(GN_FWD_APPLY, B, HW, C / V);     // (256 ... 1024 blocks and 2 / 4 / 8 rows in flight per thread
    gn_dispatch_slots(C / V, [&](auto slots) {                  //  measure the same, tools/gn_dbg.py)
        hipLaunchKernelGGL((gn_apply_kernel<T, GN_FWD_APPLY.unr, decltype(slots)::value>), gap.grid, dim3(NT), 0, st, (const T*)x,
                           (T*)y, gamma, beta, reinterpret_cast<const float*>(colstat), -1, stats, HW, C, ldx, ldy, G, gs, eps,
                           silu, gap.rpb, cs_ld);
    });
    PDMK_CHECK_LAUNCH();
    return 0;
}

template <typename T>
int gn_bwd(const void* x, const void* dy, void* dx, const float* gamma, const float* beta, const float* stats,
           float* dgamma, float* dbeta, double* ws, float* part, long part_elems, int B, int HW, int C, int ldx,
           int lddy, int lddx, int G, int gs, int silu, int acc, const void* add, int ldadd, hipStream_t st) {
    constexpr int V = Vec<T>::N;
    if (!gn_shape_ok<V>(C, G, gs, {ldx, lddy, lddx}, true)) return -1;
    if (add && ((ldadd % V) || ((uintptr_t)add & 15))) return -1;
    const GnGrid gst = gn_grid(GN_BWD_STATS, B, HW, C / V), gap = gn_grid(GN_BWD_APPLY, B, HW, C / V);
    const int nblk = gst.grid.x * gst.grid.y, cr = G * gs;
    if (!part || (long)nblk * 2 * cr > part_elems) return -1;
    float* gpart = reinterpret_cast<float*>(ws);                    // [B][nblk][G][2] floats <= B*G*64 doubles
    gn_dispatch_slots(C / V, [&](auto slots) {
        constexpr int S = decltype(slots)::value;
        hipLaunchKernelGGL((gn_bwd_stats_kernel<T, GN_BWD_STATS.unr, S>), gst.grid, dim3(NT), 0, st, (const T*)x, (const T*)dy,
                           gamma, beta, stats, part, gpart, HW, C, ldx, lddy, G, gs, silu, gst.rpb);
        launch_reduce_partials(part, nblk, cr, dgamma, dbeta, st);
        hipLaunchKernelGGL((gn_bwd_apply_kernel<T, GN_BWD_APPLY.unr, S>), gap.grid, dim3(NT), 0, st, (const T*)x, (const T*)dy,
                           (T*)dx, gamma, beta, stats, gpart, (int)gst.grid.x, HW, C, ldx, lddy, lddx, G, gs, silu, acc, gap.rpb,
                           (const T*)add, ldadd);
    });
    PDMK_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------ LayerNorm
constexpr int LN_MAXS = 5;   // per-lane chunk slots: C <= 5*64*chunk

// forward: a wave owns `rows_per_wave` consecutive rows.  gamma / beta stay in registers for all of them (16-byte loads, once per
// wave: the first version re-read them element by element for every row - 16 scalar loads per lane and row against one 16-byte
// load and one store of data, so the kernel was bound by VMEM instruction issue, 3.7 TB/s where a copy reaches 6.4) and the next
// row's load is in flight while the current row is reduced and written (the two wave reductions make one row a latency chain).
template <typename T, int SLOTS>
__global__ __launch_bounds__(NT) void ln_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float* __restrict__ stats, int M, int C, int ldx, int ldy,
                                                    float eps, int rows_per_wave) {
    constexpr int V = Vec<T>::N;
    typedef typename Vec<T>::raw Raw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mbase = (blockIdx.x * 4 + wave) * rows_per_wave, mend = min(M, mbase + rows_per_wave);
    if (mbase >= M) return;
    const int nchunks = C / V;
    const bool vec_gb = ((reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta)) & 15) == 0;
    Raw pre[SLOTS];
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        const int c = lane + 64 * sl;
        if (c < nchunks) pre[sl] = Vec<T>::load_raw(x + (long)mbase * ldx + c * V);
    }
    float gm[SLOTS][V], bt[SLOTS][V];
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        const int c = lane + 64 * sl;
        if (c < nchunks && vec_gb) {
#pragma unroll
            for (int e = 0; e < V; e += 4) {
                const float4 g4 = *reinterpret_cast<const float4*>(gamma + c * V + e), b4 = *reinterpret_cast<const float4*>(beta + c * V + e);
                gm[sl][e] = g4.x; gm[sl][e + 1] = g4.y; gm[sl][e + 2] = g4.z; gm[sl][e + 3] = g4.w;
                bt[sl][e] = b4.x; bt[sl][e + 1] = b4.y; bt[sl][e + 2] = b4.z; bt[sl][e + 3] = b4.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                gm[sl][e] = c < nchunks ? gamma[c * V + e] : 0.f;
                bt[sl][e] = c < nchunks ? beta[c * V + e] : 0.f;
            }
        }
    }
    const float invC = 1.0f / C;
    for (int m = mbase; m < mend; ++m) {
        float f[SLOTS][V];
        float sum = 0.f;
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            const int c = lane + 64 * sl;
            if (c < nchunks) {
                Vec<T>::unpack(pre[sl], f[sl]);
                if (m + 1 < mend) pre[sl] = Vec<T>::load_raw(x + (long)(m + 1) * ldx + c * V);
#pragma unroll
                for (int e = 0; e < V; ++e) sum += f[sl][e];
            }
        }
        const float mean = wave_sum(sum) * invC;
        float sq = 0.f;
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            const int c = lane + 64 * sl;
            if (c < nchunks) {
#pragma unroll
                for (int e = 0; e < V; ++e) { const float d = f[sl][e] - mean; sq += d * d; }
            }
        }
        const float rstd = rsqrtf(wave_sum(sq) * invC + eps);
        if (lane == 0) { stats[2 * (long)m] = mean; stats[2 * (long)m + 1] = rstd; }
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            const int c = lane + 64 * sl;
            if (c < nchunks) {
                float o[V];
#pragma unroll
                for (int e = 0; e < V; ++e) o[e] = (f[sl][e] - mean) * rstd * gm[sl][e] + bt[sl][e];
                Vec<T>::store(y + (long)m * ldy + c * V, o);
            }
        }
    }
}

// backward: a row is owned by a group of L lanes (L = 8 / 16 / 32 / 64 chosen from C so that a lane holds S <= 5 16-byte chunks,
// ln_bwd_form), so a wave works on G = 64 / L rows per pass and the four waves of a block on 4 * G consecutive rows: lane
// (grp, li) of wave w holds chunks li, li + L, ... of row r0 + (pass * 4 + w) * G + grp - each wave load instruction covers G
// pieces of L * 16 contiguous bytes (>= one 128-byte segment).  One wave per row (the previous form) left 24 of 64 lanes without
// a chunk at C = 320, paid two 6-step wave reductions per row and two broadcast dword loads of the row statistics per lane and
// row, and read gamma element by element.  Here
//  - the two row sums are log2(L) exchange steps that serve all G rows of the wave at once, (mean, rstd) is one 8-byte load;
//  - gamma is read once per block (coalesced dwords, issued before the rows) into LDS and taken from there as float4 at each
//    use: S * V registers less than a register copy, which is what lets the S = 3 forms run two waves per SIMD;
//  - x, dy and the statistics of the next pass are requested before the current pass is reduced (register double buffer);
//    the `add` and accumulate_dx operands, when present, go out with the first pass's rows and after that as soon as the
//    pass that used their registers has stored (a second register set for them costs the second wave per SIMD);
//  - x and dy stay packed between their two uses (row sums, then dx): unpacking twice is cheaper than S * V * 2 live floats;
//  - dgamma / dbeta: per lane over all its rows, then across the wave's G row groups in registers, then across the four waves
//    in LDS in a fixed order, one slab row per block written by all 256 threads (no atomics: the slab is bit-reproducible).
// S = 5 (which C = 320 / 640 / 1280 would fit with L = 8 / 16 / 32) takes 357 registers - one wave per SIMD - and measured slower
// than S = 3 on twice the lanes at every step shape (32 768 x 320: 34.7 against 24.7 us in one session), so S = 5 is left to C > 1536 (bf16);
// profiles/ln_bwd_bench.txt has the A/B against the one-wave-per-row kernel.
// the packed chunk is used twice (row sums, then dx); without this the compiler keeps the unpacked floats of the first use alive
template <typename R> __device__ __forceinline__ void keep_packed(R& r) {
    f32x4 t = __builtin_bit_cast(f32x4, r);
    asm volatile("" : "+v"(t));
    r = __builtin_bit_cast(R, t);
}
template <typename T, int L, int S>
__global__ __launch_bounds__(NT) void ln_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                    T* __restrict__ dx, const float* __restrict__ gamma,
                                                    const float* __restrict__ stats, float* __restrict__ part,
                                                    int M, int C, int ldx, int lddy,
                                                    int lddx, int accumulate, int rows_per_blk,
                                                    const T* __restrict__ add, int ldadd) {
    // add (optional): a second finished gradient of the same tensor (the residual branch's, blocks.py:705-867) added in this
    // store - dx = (accumulate ? dx : 0) + add + this layer's input gradient - so that the fan-in needs neither a pass of its
    // own nor an in-place update of a buffer another kernel still reads (a deferred weight gradient's dY)
    constexpr int V = Vec<T>::N, G = 64 / L, LV = L * V;
    typedef typename Vec<T>::raw Raw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane % L, grp = lane / L;
    const int nchunks = C / V;
    const int r0 = blockIdx.x * rows_per_blk, r1 = min(M, r0 + rows_per_blk);      // r0 < M: the grid is ceil(M / rows_per_blk)
    __shared__ __attribute__((aligned(16))) float sgm[S * LV];     // gamma, zero past C
    __shared__ float red[2][4][LV];
    float gst[(S * LV + NT - 1) / NT];
#pragma unroll
    for (int i = 0; i < (S * LV + NT - 1) / NT; ++i) {             // (first: loads return in issue order, and the rows follow)
        const int col = threadIdx.x + i * NT;
        gst[i] = col < C ? gamma[col] : 0.f;
    }
    // loads carry no lane condition (a branch around each one serialises them): a chunk slot past the row re-reads the row's
    // first chunk, and its gamma is zero, so it adds nothing to the row sums; its column sums and its dx are never stored
    int coff[S];
#pragma unroll
    for (int sl = 0; sl < S; ++sl) coff[sl] = (li + L * sl < nchunks ? li + L * sl : 0) * V;
    Raw px[S], pd[S], pa[S], po[S];
    float2 pst;
#pragma unroll
    for (int sl = 0; sl < S; ++sl) pa[sl] = po[sl] = Raw{};
    auto fetch_xd = [&](int m0) {
        const long m = min(m0 + grp, r1 - 1);             // clamp: duplicates of the block's last row are discarded below
        pst = *reinterpret_cast<const float2*>(stats + 2 * m);
        const T *xr = x + m * ldx, *dr = dy + m * lddy;
#pragma unroll
        for (int sl = 0; sl < S; ++sl) {
            px[sl] = Vec<T>::load_raw(xr + coff[sl]);
            pd[sl] = Vec<T>::load_raw(dr + coff[sl]);
        }
    };
    auto fetch_ao = [&](int m0) {
        const long m = min(m0 + grp, r1 - 1);
        if (add) {
            const T* ar = add + m * ldadd;
#pragma unroll
            for (int sl = 0; sl < S; ++sl) pa[sl] = Vec<T>::load_raw(ar + coff[sl]);
        }
        if (accumulate) {
            const T* orow = dx + m * lddx;
#pragma unroll
            for (int sl = 0; sl < S; ++sl) po[sl] = Vec<T>::load_raw(orow + coff[sl]);
        }
    };
    int m0 = r0 + wave * G;
    if (m0 < r1) { fetch_xd(m0); fetch_ao(m0); }
    else {
#pragma unroll
        for (int sl = 0; sl < S; ++sl) px[sl] = pd[sl] = Raw{};
        pst = float2{0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < (S * LV + NT - 1) / NT; ++i) {
        const int col = threadIdx.x + i * NT;
        if (col < S * LV) sgm[col] = gst[i];
    }
    __syncthreads();
    float ag[S][V], ab[S][V];
#pragma unroll
    for (int sl = 0; sl < S; ++sl)
#pragma unroll
        for (int e = 0; e < V; ++e) ag[sl][e] = ab[sl][e] = 0.f;
    auto load_gm = [&](int sl, float* gm) {
#pragma unroll
        for (int e = 0; e < V; e += 4) {
            const float4 g4 = *reinterpret_cast<const float4*>(&sgm[(li + L * sl) * V + e]);
            gm[e] = g4.x; gm[e + 1] = g4.y; gm[e + 2] = g4.z; gm[e + 3] = g4.w;
        }
    };
    const float invC = 1.0f / C;
    for (; m0 < r1; m0 += 4 * G) {                       // (wave-uniform: no barrier inside)
        Raw cx[S], cd[S];
#pragma unroll
        for (int sl = 0; sl < S; ++sl) { cx[sl] = px[sl]; cd[sl] = pd[sl]; }
        const float mean = pst.x, rstd = pst.y;
        const bool more = m0 + 4 * G < r1;
        if (more) fetch_xd(m0 + 4 * G);
        const bool live = m0 + grp < r1;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int sl = 0; sl < S; ++sl) {
            float f[V], d[V], gm[V];
            Vec<T>::unpack(cx[sl], f);
            Vec<T>::unpack(cd[sl], d);
            load_gm(sl, gm);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float h = (f[e] - mean) * rstd;
                if (live) { ab[sl][e] += d[e]; ag[sl][e] += d[e] * h; }
                const float g = d[e] * gm[e];            // (chunk slots past the row: gm = 0)
                s1 += g;
                s2 += g * h;
            }
        }
#pragma unroll
        for (int o = L / 2; o > 0; o >>= 1) {
            s1 += __shfl_xor(s1, o, 64);
            s2 += __shfl_xor(s2, o, 64);
        }
        s1 *= invC;
        s2 *= invC;
        if (live) {
            const long m = m0 + grp;
#pragma unroll
            for (int sl = 0; sl < S; ++sl) {
                const int c = li + L * sl;
                if (c < nchunks) {
                    float f[V], d[V], gm[V], o[V];
                    keep_packed(cx[sl]);
                    keep_packed(cd[sl]);
                    Vec<T>::unpack(cx[sl], f);
                    Vec<T>::unpack(cd[sl], d);
                    load_gm(sl, gm);
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const float h = (f[e] - mean) * rstd;
                        o[e] = rstd * (d[e] * gm[e] - s1 - h * s2);
                    }
                    if (add) {                           // (uniform branches: the plain form pays nothing for the operands)
                        float a2[V];
                        Vec<T>::unpack(pa[sl], a2);
#pragma unroll
                        for (int e = 0; e < V; ++e) o[e] += a2[e];
                    }
                    if (accumulate) {
                        float o2[V];
                        Vec<T>::unpack(po[sl], o2);
#pragma unroll
                        for (int e = 0; e < V; ++e) o[e] = o2[e] + o[e];
                    }
                    Vec<T>::store(dx + m * lddx + c * V, o);
                }
            }
        }
        if (more) fetch_ao(m0 + 4 * G);
    }
    // column sums: across the wave's G row groups in registers (every lane ends with the same sum), then the four waves in LDS,
    // a slot at a time, in a fixed order; all 256 threads write the slab row (second stage: reduce_partials_kernel)
    float* slab = part + (long)blockIdx.x * 2 * C;          // [dgamma | dbeta] of this block
#pragma unroll
    for (int sl = 0; sl < S; ++sl) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
#pragma unroll
            for (int o = L; o < 64; o <<= 1) {
                ag[sl][e] += __shfl_xor(ag[sl][e], o, 64);
                ab[sl][e] += __shfl_xor(ab[sl][e], o, 64);
            }
        }
        __syncthreads();
        if (lane < L) {
#pragma unroll
            for (int e = 0; e < V; ++e) { red[0][wave][lane * V + e] = ag[sl][e]; red[1][wave][lane * V + e] = ab[sl][e]; }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < 2 * LV; j += NT) {
            const int w = j / LV, jj = j - w * LV, col = sl * LV + jj;
            if (col < C) slab[w * C + col] = (red[w][0][jj] + red[w][1][jj]) + (red[w][2][jj] + red[w][3][jj]);
        }
    }
}

template <typename T>
int ln_fwd(const void* x, void* y, const float* gamma, const float* beta, float* stats, int M, int C, int ldx, int ldy,
           float eps, hipStream_t st) {
    constexpr int V = Vec<T>::N;
    if (C % V || ldx % V || ldy % V || C / V > LN_MAXS * 64) return -1;
    int rpw = M / 8192;                              // rows per wave: 1 ... 8, >= ~2048 blocks of 4 waves (tools/ln_bench.py: 32 768 x 320
    rpw = rpw < 1 ? 1 : (rpw > 8 ? 8 : rpw);         // rows take 13.6 / 12.2 / 11.6 / 14.6 us at 1 / 2 / 4 / 8 rows per wave)
    const dim3 grid((M + 4 * rpw - 1) / (4 * rpw));
    const int slots = (C / V + 63) / 64;
#define PDMK_LNF(S) hipLaunchKernelGGL((ln_fwd_kernel<T, S>), grid, dim3(NT), 0, st, (const T*)x, (T*)y, gamma, beta, stats, M, \
                                       C, ldx, ldy, eps, rpw)
    if (slots == 1) PDMK_LNF(1);
    else if (slots == 2) PDMK_LNF(2);
    else if (slots == 3) PDMK_LNF(3);
    else PDMK_LNF(5);
#undef PDMK_LNF
    PDMK_CHECK_LAUNCH();
    return 0;
}
// rows per block of the LayerNorm backward: as many blocks as 16 rows per block allow, up to 512 (also fixes the partial-slab
// count: pdmk_layernorm_bwd_partial_dims and the launch both call this, and pdmk.h promises M / 16 + 1 slabs are enough).
// Above 16 the count is a multiple of 32 - whole passes of every lane-group form (a block pass is 4 * 64 / L <= 32 rows) - and at
// most 256.  8192 x 640 -> 512 blocks, 2048 x 1280 -> 128, 512 x 1280 -> 32, 32 768 x 320 -> 512 of 64 rows, 65 536 x 320 -> 512
// of 128 rows.  (The one-wave-per-row kernel never went below 32 rows: its LDS combine and slab row cost ~16 rows of streaming
// and 2048 x 1280 ran on 64 of the 256 CUs; the A/B of this rule and kernel is profiles/ln_bwd_bench.txt.)
static int ln_bwd_rows_per_blk(int M) {
    const int rpb = (M + 511) / 512;
    if (rpb <= 16) return 16;
    return rpb > 224 ? 256 : (rpb + 31) / 32 * 32;
}
// lane-group form from the chunk count alone: L lanes per row, S chunks per lane (L * S >= nchunks, S <= LN_MAXS)
struct LnBwdForm {
    int L, S;
};
static LnBwdForm ln_bwd_form(int nchunks) {
    if (nchunks <= 8) return {8, 1};
    if (nchunks <= 16) return {8, 2};
    if (nchunks <= 24) return {8, 3};
    if (nchunks <= 48) return {16, 3};
    if (nchunks <= 96) return {32, 3};
    if (nchunks <= 192) return {64, 3};
    return {64, 5};
}
template <typename T>
int ln_bwd(const void* x, const void* dy, void* dx, const float* gamma, const float* stats, float* dgamma,
           float* dbeta, float* part, long part_elems, int M, int C, int ldx, int lddy, int lddx, int acc,
           const void* add, int ldadd, hipStream_t st) {
    constexpr int V = Vec<T>::N;
    if (C % V || ldx % V || lddy % V || lddx % V || C / V > LN_MAXS * 64 || (add && (ldadd % V))) return -1;
    const int rows_per_blk = ln_bwd_rows_per_blk(M);
    const dim3 grid((M + rows_per_blk - 1) / rows_per_blk);
    if (!part || (long)grid.x * 2 * C > part_elems) return -1;
    const LnBwdForm fm = ln_bwd_form(C / V);
#define PDMK_LNB(LL, SS) hipLaunchKernelGGL((ln_bwd_kernel<T, LL, SS>), grid, dim3(NT), 0, st, (const T*)x, (const T*)dy, \
                                            (T*)dx, gamma, stats, part, M, C, ldx, lddy, lddx, acc, rows_per_blk,       \
                                            (const T*)add, ldadd)
    if (fm.L == 8 && fm.S == 1) PDMK_LNB(8, 1);
    else if (fm.L == 8 && fm.S == 2) PDMK_LNB(8, 2);
    else if (fm.L == 8) PDMK_LNB(8, 3);
    else if (fm.L == 16) PDMK_LNB(16, 3);
    else if (fm.L == 32) PDMK_LNB(32, 3);
    else if (fm.S == 3) PDMK_LNB(64, 3);
    else PDMK_LNB(64, 5);
#undef PDMK_LNB
    launch_reduce_partials(part, grid.x, C, dgamma, dbeta, st);
    PDMK_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int pdmk_groupnorm_apply_colstat(const void* x, void* y, const float* gamma, const float* beta, float* stats,
                                            const int64_t* colstat, int cs_ld, int cs_col0, int B, int HW, int C, int ldx, int ldy,
                                            int G, int gs, float eps, int silu, int dtype, pdmk_stream stream) {
    if (!x || !y || !gamma || !beta || !stats || !colstat || B <= 0 || HW <= 0 || C <= 0 || G <= 0 || gs <= 0 || cs_col0 < 0 ||
        cs_ld < cs_col0 + G * gs)
        return -1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == PDMK_BF16) return gn_apply_colstat<bf16>(x, y, gamma, beta, stats, colstat + cs_col0, cs_ld, B, HW, C, ldx, ldy, G, gs, eps, silu, st);
    if (dtype == PDMK_F32) return gn_apply_colstat<float>(x, y, gamma, beta, stats, colstat + cs_col0, cs_ld, B, HW, C, ldx, ldy, G, gs, eps, silu, st);
    return -2;
}

extern "C" int pdmk_groupnorm_fwd(const void* x, void* y, const float* gamma, const float* beta, float* stats,
                                  double* ws, int B, int HW, int C, int ldx, int ldy, int G, int gs, float eps,
                                  int silu, int dtype, pdmk_stream stream) {
    if (!x || !y || !gamma || !beta || !stats || !ws || B <= 0 || HW <= 0 || G <= 0 || gs <= 0) return -1;
    PDMK_DISPATCH(dtype, gn_fwd, x, y, gamma, beta, stats, ws, B, HW, C, ldx, ldy, G, gs, eps, silu,
                  (hipStream_t)stream);
}
extern "C" int pdmk_groupnorm_bwd(const void* x, const void* dy, void* dx, const float* gamma, const float* beta,
                                  const float* stats, float* dgamma, float* dbeta, double* ws, float* part_ws,
                                  int64_t part_ws_elems, int B, int HW, int C, int ldx, int lddy, int lddx, int G,
                                  int gs, int silu, int accumulate_dx, const void* add, int ldadd, int dtype,
                                  pdmk_stream stream) {
    if (!x || !dy || !dx || !gamma || !beta || !stats || (!dgamma != !dbeta) || !ws || B <= 0 || HW <= 0) return -1;
    PDMK_DISPATCH(dtype, gn_bwd, x, dy, dx, gamma, beta, stats, dgamma, dbeta, ws, part_ws, (long)part_ws_elems, B, HW,
                  C, ldx, lddy, lddx, G, gs, silu, accumulate_dx, add, ldadd, (hipStream_t)stream);
}
/* Slab geometry of the parameter-gradient partials the two backward passes leave in part_ws ([nblk][2][n] floats). */
extern "C" int pdmk_groupnorm_bwd_partial_dims(int B, int HW, int C, int G, int gs, int dtype, int32_t* nblk, int32_t* n) {
    if (!nblk || !n || B <= 0 || HW <= 0 || C <= 0) return -1;
    const int V = dtype == PDMK_BF16 ? 8 : 4;
    if (C % V) return -1;
    const dim3 grid = gn_grid(GN_BWD_STATS, B, HW, C / V).grid;    // the grid gn_bwd launches and checks part_ws_elems against
    *nblk = grid.x * grid.y;
    *n = G * gs;
    return 0;
}
extern "C" int pdmk_layernorm_bwd_partial_dims(int M, int C, int32_t* nblk, int32_t* n) {
    if (!nblk || !n || M <= 0 || C <= 0) return -1;
    const int rpb = ln_bwd_rows_per_blk(M);
    *nblk = (M + rpb - 1) / rpb;
    *n = C;
    return 0;
}
extern "C" int pdmk_reduce_partials_group(const pdmk_partial_item* items, int n_items, pdmk_stream stream) {
    if (!items || n_items <= 0 || n_items > PDMK_PARTIAL_GROUP_MAX) return -1;
    PartialGroup gr;
    int nmax = 0;
    for (int i = 0; i < n_items; ++i) {
        if (!items[i].part || !items[i].out0 || !items[i].out1 || items[i].nblk <= 0 || items[i].n <= 0) return -1;
        gr.it[i] = items[i];
        nmax = items[i].n > nmax ? items[i].n : nmax;
    }
    for (int i = n_items; i < PDMK_PARTIAL_GROUP_MAX; ++i) gr.it[i] = items[0];
    hipLaunchKernelGGL(reduce_partials_group_kernel, dim3((2 * nmax + NT - 1) / NT, n_items * 8), dim3(NT), 0,
                       (hipStream_t)stream, gr);
    PDMK_CHECK_LAUNCH();
    return 0;
}
extern "C" int pdmk_layernorm_fwd(const void* x, void* y, const float* gamma, const float* beta, float* stats, int M,
                                  int C, int ldx, int ldy, float eps, int dtype, pdmk_stream stream) {
    if (!x || !y || !gamma || !beta || !stats || M <= 0) return -1;
    PDMK_DISPATCH(dtype, ln_fwd, x, y, gamma, beta, stats, M, C, ldx, ldy, eps, (hipStream_t)stream);
}
extern "C" int pdmk_layernorm_bwd(const void* x, const void* dy, void* dx, const float* gamma, const float* stats,
                                  float* dgamma, float* dbeta, float* part_ws, int64_t part_ws_elems, int M, int C,
                                  int ldx, int lddy, int lddx, int accumulate_dx, const void* add, int ldadd, int dtype,
                                  pdmk_stream stream) {
    if (!x || !dy || !dx || !gamma || !stats || (!dgamma != !dbeta) || M <= 0) return -1;
    PDMK_DISPATCH(dtype, ln_bwd, x, dy, dx, gamma, stats, dgamma, dbeta, part_ws, (long)part_ws_elems, M, C, ldx, lddy,
                  lddx, accumulate_dx, add, ldadd, (hipStream_t)stream);
}
