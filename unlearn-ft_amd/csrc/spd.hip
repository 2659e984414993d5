// Dense symmetric-positive-definite solve in fp64 and the target differences of the closed-form cross-attention edit
// (include/pdmk.h "UCE"; pdm/utils/uce.py):
//   pdmk_spd_system_f64 : A = lam I + s_a sym(g_a) + s_b sym(g_b) from the Gram matrices pdmk_fid_accumulate leaves
//   pdmk_pair_gram_f64  : A = lam I + scale sum_p delta_p delta_p^T from pairs of fp32 rows (debias-VL's calibration matrix)
//   pdmk_spd_factor_f64 : blocked right-looking Cholesky A = L L^T in place, 64-wide panels, three launches per panel
//   pdmk_spd_solve_f64  : X = B (L L^T)^-1 for the rows of B, forward then backward block substitution per block of 16 rows
//   pdmk_uce_delta      : D = N - O (replace) or N - (1 + <O, N> / <O, O>) O per (pair, projection) block (tensor)
//   pdmk_uce_debias_delta : D = sum_j c_j U_j per block, c_j from the debiasing recurrence on the block's Gram matrix
//
// Every triangular system against a 64 x 64 diagonal block is solved by substitution (one division per element), never by a
// product with an explicit inverse: the componentwise error bounds of Cholesky factorisation and of the
// triangular solves (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3 / 10.4) hold for substitution in any
// order of summation, and the tests hold the kernels to exactly these bounds; a product with a computed inverse would carry
// the condition number of the diagonal block.  All products are plain fp64 FMAs.
//
// Nothing here allocates, waits on the host or uses an atomic; one panel's dependence on the previous one is a launch
// boundary on the stream, and inside a launch no workgroup reads what another one writes.  Every sum has one fixed order, so
// the same inputs give the same bits, and a row of the solve does not depend on which rows share its block.
#include <float.h>

#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int NB = 64;            // panel width = side of a diagonal block
constexpr int LS = NB + 1;        // LDS row stride of a staged block (doubles): column reads touch 64 different banks
constexpr int RB = 16;            // rows of B per workgroup of the solve
constexpr int UK = 16;            // panel columns staged per step of the trailing update

// ---------------------------------------------------------------------------------------------------- system
// Element (i, j) of sym(g) comes from the 64 x 64 tile that pdmk_fid_accumulate wrote: tile (i / 64, j / 64) when its row is
// not below its column, else the mirrored element.
__global__ void __launch_bounds__(NT) spd_system_kernel(const double* __restrict__ ga, double sa, const double* __restrict__ gb,
                                                        double sb, double lam, double* __restrict__ A, int n, int lda) {
    const long total = (long)n * n;
    for (long e = (long)blockIdx.x * NT + threadIdx.x; e < total; e += (long)gridDim.x * NT) {
        const int i = (int)(e / n), j = (int)(e - (long)i * n);
        const long src = (i / NB <= j / NB) ? (long)i * n + j : (long)j * n + i;
        double v = fma(sa, ga[src], i == j ? lam : 0.0);
        if (gb) v = fma(sb, gb[src], v);
        A[(long)i * lda + j] = v;
    }
}

// Debias-VL's calibration matrix (include/pdmk.h pdmk_pair_gram_f64): one workgroup per 64 x 64 tile of A, the differences
// delta_p of PG pairs at a time staged in LDS for the tile's rows and columns (zeros past npairs and past d, which add nothing),
// a 4 x 4 block of sums per thread (rows ty + 16 a, columns tx + 16 b: the column reads of a wave are consecutive, the row reads a
// broadcast).  Each sum is one chain of fp64 FMAs over p ascending.
constexpr int PG = 16;
__global__ void __launch_bounds__(NT) pair_gram_kernel(const float* __restrict__ z, int ldz, int npairs, int d, double scale,
                                                       double lam, double* __restrict__ A, int lda) {
    __shared__ double di[PG][NB], dj[PG][NB];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * NB, j0 = blockIdx.x * NB;
    double acc[4][4] = {};
    for (int p0 = 0; p0 < npairs; p0 += PG) {
        for (int idx = tid; idx < PG * NB; idx += NT) {
            const int pp = idx / NB, col = idx - pp * NB, p = p0 + pp;
            const float* male = z + (long)(2 * p) * ldz;
            const float* female = male + ldz;
            const bool in = p < npairs;
            di[pp][col] = in && i0 + col < d ? (double)male[i0 + col] - (double)female[i0 + col] : 0.0;
            dj[pp][col] = in && j0 + col < d ? (double)male[j0 + col] - (double)female[j0 + col] : 0.0;
        }
        __syncthreads();
        for (int pp = 0; pp < PG; ++pp) {
            double r[4], c[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) r[a] = di[pp][ty + 16 * a], c[a] = dj[pp][tx + 16 * a];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(r[a], c[b], acc[a][b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i < d && j < d) A[(long)i * lda + j] = fma(scale, acc[a][b], i == j ? lam : 0.0);
        }
}

// ---------------------------------------------------------------------------------------------------- factor
// Launch 1 of panel j0: the diagonal block (w = min(64, n - j0) real columns, identity beyond them) is factored in LDS by one
// workgroup, column by column: pivot check and square root, column scaled, the columns right of it updated.
__global__ void __launch_bounds__(NT) chol_diag_kernel(double* __restrict__ A, int n, int lda, int j0, int32_t* __restrict__ info) {
    __shared__ double T[NB * LS];
    const int tid = threadIdx.x;
    const int w = min(NB, n - j0);
    for (int e = tid; e < NB * NB; e += NT) {
        const int r = e >> 6, c = e & 63;
        double v = r == c ? 1.0 : 0.0;
        if (c <= r && r < w) v = A[(long)(j0 + r) * lda + j0 + c];
        T[r * LS + c] = v;
    }
    const int r = tid >> 2, kq = tid & 3;                     // trailing update: row r, columns c + 1 + kq, + 4, ...
    for (int c = 0; c < w; ++c) {
        __syncthreads();
        const double p = T[c * LS + c];
        if (tid == 0 && !(p > 0.0 && p <= DBL_MAX) && *info == 0) *info = j0 + c + 1;
        const double d = sqrt(p);
        __syncthreads();                                      // every thread has read the pivot
        if (tid == 0) T[c * LS + c] = d;
        if (tid > c && tid < NB) T[tid * LS + c] = T[tid * LS + c] / d;
        __syncthreads();
        if (r > c) {
            const double lr = T[r * LS + c];
            for (int k = c + 1 + kq; k <= r; k += 4) T[r * LS + k] = fma(-lr, T[k * LS + c], T[r * LS + k]);
        }
    }
    __syncthreads();
    for (int e = tid; e < NB * NB; e += NT) {
        const int rr = e >> 6, c = e & 63;
        if (c <= rr && rr < w) A[(long)(j0 + rr) * lda + j0 + c] = T[rr * LS + c];
    }
}

// Launch 2: the rows below the diagonal block, one thread per row: x L_jj^T = a by forward substitution against the block in
// LDS (every lane reads the same element: a broadcast), the row in registers.  Only launched when rows exist below, so the
// diagonal block has all 64 columns.
__global__ void __launch_bounds__(NT) chol_panel_kernel(double* __restrict__ A, int n, int lda, int j0) {
    __shared__ double Ld[NB * LS];
    for (int e = threadIdx.x; e < NB * NB; e += NT) {
        const int r = e >> 6, c = e & 63;
        if (c <= r) Ld[r * LS + c] = A[(long)(j0 + r) * lda + j0 + c];
    }
    __syncthreads();
    const int row = j0 + NB + blockIdx.x * NT + threadIdx.x;
    if (row >= n) return;
    double* a = A + (long)row * lda + j0;
    double x[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        double s = a[c];
#pragma unroll
        for (int q = 0; q < c; ++q) s = fma(-x[q], Ld[c * LS + q], s);
        x[c] = s / Ld[c * LS + c];
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) a[c] = x[c];
}

// Launch 3: A_ik -= L_ij L_kj^T for every 64 x 64 tile (i, k), k <= i, of the trailing matrix (a diagonal tile is updated
// whole).  Thread (ty, tx) of 16 x 16 owns rows 4 ty + a, columns tx + 16 c, as pdmk_fid_accumulate.  The tiles read columns
// j0 .. j0 + 63 and write columns >= j0 + 64: no workgroup reads another one's output.
__global__ void __launch_bounds__(NT) chol_update_kernel(double* __restrict__ A, int n, int lda, int j0) {
    __shared__ double Pi[UK][LS], Pk[UK][LS];
    const int r0 = j0 + NB;
    int ti = 0, rem = blockIdx.x;                             // linear id -> (ti, tk) of the lower triangle, row by row
    while (rem > ti) {
        rem -= ti + 1;
        ++ti;
    }
    const int i0 = r0 + ti * NB, k0 = r0 + rem * NB;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + 4 * ty + a, k = k0 + tx + 16 * c;
            acc[a][c] = (i < n && k < n) ? A[(long)i * lda + k] : 0.0;
        }
    for (int q0 = 0; q0 < NB; q0 += UK) {
        __syncthreads();
        for (int e = threadIdx.x; e < UK * NB; e += NT) {
            const int r = e >> 4, q = e & 15;
            Pi[q][r] = i0 + r < n ? A[(long)(i0 + r) * lda + j0 + q0 + q] : 0.0;
            Pk[q][r] = k0 + r < n ? A[(long)(k0 + r) * lda + j0 + q0 + q] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < UK; ++q) {
            double u[4], v[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) u[a] = Pi[q][4 * ty + a];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = Pk[q][tx + 16 * c];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] = fma(-u[a], v[c], acc[a][c]);
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + 4 * ty + a, k = k0 + tx + 16 * c;
            if (i < n && k < n) A[(long)i * lda + k] = acc[a][c];
        }
}

// ---------------------------------------------------------------------------------------------------- solve
// S[a][b] = L[rb + a][cb + b]; outside the matrix (and, for a diagonal block, above the diagonal, which is never read from
// memory) the identity.
__device__ __forceinline__ void stage_block(double* S, const double* __restrict__ L, int n, int ldl, int rb, int cb, bool diag) {
    for (int e = threadIdx.x; e < NB * NB; e += NT) {
        const int a = e >> 6, b = e & 63;
        const int i = rb + a, j = cb + b;
        double v = (diag && a == b) ? 1.0 : 0.0;
        if (i < n && j < n && (!diag || b <= a)) v = L[(long)i * ldl + j];
        S[a * LS + b] = v;
    }
}

// The RB x 64 block in Ts against the diagonal block in S: T L^-T (FWD: y_c = (t_c - sum_{q<c} y_q L[c][q]) / L[c][c], columns
// ascending) or T L^-1 (x_c = (t_c - sum_{q>c} x_q L[q][c]) / L[c][c], columns descending), column by column: every thread of row
// r = tid / 16 forms the finished element itself, then the 16 of them subtract its multiple from the row's open columns (thread
// l: columns l, l + 16, ...).  The result goes to Ys.  Each element receives its terms in a fixed order, whatever the row.
template <bool FWD>
__device__ __forceinline__ void diag_substitute(const double* S, double (*Ts)[LS], double (*Ys)[NB]) {
    const int r = threadIdx.x >> 4, l = threadIdx.x & 15;
    for (int s = 0; s < NB; ++s) {
        const int cc = FWD ? s : NB - 1 - s;
        const double x = Ts[r][cc] / S[cc * LS + cc];
        if (l == (cc & 15)) Ys[r][cc] = x;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = l + 16 * i;
            if (FWD ? c > cc : c < cc) Ts[r][c] = fma(-x, FWD ? S[c * LS + cc] : S[cc * LS + c], Ts[r][c]);
        }
        __syncthreads();
    }
}

// One workgroup per RB rows of B.  Y L^T = B block column by block column (Y_j = (B_j - sum_{k<j} Y_k L_jk^T) L_jj^-T), then
// X L = Y from the last block column back (X_j = (Y_j - sum_{k>j} X_k L_kj) L_jj^-1).  The off-diagonal products are tile
// products (thread: column c of the block, rows 4 rg + a; the sum runs over k and inside k in a fixed order), the diagonal
// block is a substitution (diag_substitute).  Y and then X live in the workgroup's own RB x np rows of ws.
__global__ void __launch_bounds__(NT) spd_solve_kernel(const double* __restrict__ L, int n, int ldl, const float* __restrict__ B, int m,
                                                       int ldb, float* __restrict__ X, int ldx, double* __restrict__ X64, int ldx64,
                                                       double* __restrict__ ws) {
    __shared__ double S[NB * LS];
    __shared__ double Ys[RB][NB];
    __shared__ double Ts[RB][LS];
    const int nb = (n + NB - 1) / NB, np = nb * NB;
    const int row0 = blockIdx.x * RB;
    double* W = ws + (long)row0 * np;
    const int tid = threadIdx.x, c = tid & 63, rg = tid >> 6;
    double acc[4];

    for (int j = 0; j < nb; ++j) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int r = row0 + 4 * rg + a, col = j * NB + c;
            acc[a] = (r < m && col < n) ? (double)B[(long)r * ldb + col] : 0.0;
        }
        for (int k = 0; k < j; ++k) {
            __syncthreads();                                  // S / Ys free again; the Y blocks written so far are visible
            stage_block(S, L, n, ldl, j * NB, k * NB, false);
#pragma unroll
            for (int a = 0; a < 4; ++a) Ys[4 * rg + a][c] = W[(long)(4 * rg + a) * np + k * NB + c];
            __syncthreads();
            for (int q = 0; q < NB; ++q) {
                const double l = S[c * LS + q];
#pragma unroll
                for (int a = 0; a < 4; ++a) acc[a] = fma(-Ys[4 * rg + a][q], l, acc[a]);
            }
        }
        __syncthreads();
        stage_block(S, L, n, ldl, j * NB, j * NB, true);
#pragma unroll
        for (int a = 0; a < 4; ++a) Ts[4 * rg + a][c] = acc[a];
        __syncthreads();
        diag_substitute<true>(S, Ts, Ys);
#pragma unroll
        for (int a = 0; a < 4; ++a) W[(long)(4 * rg + a) * np + j * NB + c] = Ys[4 * rg + a][c];
    }

    for (int j = nb - 1; j >= 0; --j) {
        __syncthreads();                                      // the forward pass' last block is visible
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = W[(long)(4 * rg + a) * np + j * NB + c];
        for (int k = nb - 1; k > j; --k) {
            __syncthreads();
            stage_block(S, L, n, ldl, k * NB, j * NB, false);
#pragma unroll
            for (int a = 0; a < 4; ++a) Ys[4 * rg + a][c] = W[(long)(4 * rg + a) * np + k * NB + c];
            __syncthreads();
            for (int q = NB - 1; q >= 0; --q) {
                const double l = S[q * LS + c];
#pragma unroll
                for (int a = 0; a < 4; ++a) acc[a] = fma(-Ys[4 * rg + a][q], l, acc[a]);
            }
        }
        __syncthreads();
        stage_block(S, L, n, ldl, j * NB, j * NB, true);
#pragma unroll
        for (int a = 0; a < 4; ++a) Ts[4 * rg + a][c] = acc[a];
        __syncthreads();
        diag_substitute<false>(S, Ts, Ys);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double v = Ys[4 * rg + a][c];
            W[(long)(4 * rg + a) * np + j * NB + c] = v;
            const int r = row0 + 4 * rg + a, col = j * NB + c;
            if (r < m && col < n) {
                X[(long)r * ldx + col] = (float)v;            // round to nearest even
                if (X64) X64[(long)r * ldx64 + col] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- delta
// ws[2 (p Q + q)] = sum O N, ws[.. + 1] = sum O^2 over block (pair p, projection q): thread t takes the block's elements t,
// t + 256, ... in row-major order (products of two fp32 values are exact in fp64), then the wave butterfly and the four waves
// in order.
__global__ void __launch_bounds__(NT) uce_dot_kernel(const float* __restrict__ O, const float* __restrict__ N, int ld,
                                                     const int32_t* __restrict__ row_seg, const int32_t* __restrict__ col_seg, int Q,
                                                     double* __restrict__ ws) {
    __shared__ double red[2][NT / 64];
    const int p = blockIdx.x / Q, q = blockIdx.x - p * Q;
    const int r0 = row_seg[p], c0 = col_seg[q], w = col_seg[q + 1] - c0;
    const long cnt = (long)(row_seg[p + 1] - r0) * w;
    double a = 0.0, b = 0.0;
    for (long e = threadIdx.x; e < cnt; e += NT) {
        const long r = e / w;
        const long at = (r0 + r) * ld + c0 + (e - r * w);
        const double o = (double)O[at];
        a = fma(o, (double)N[at], a);
        b = fma(o, o, b);
    }
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[2 * (long)blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        ws[2 * (long)blockIdx.x + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// grid (Q, P + 1): block (q, p < P) writes D = N - s O over its block, s = 1 (replace) or fp32(1 + a / b) (tensor; b == 0:
// s = 1); row block P is the padding [row_seg[P], m), written as zeros.
__global__ void __launch_bounds__(NT) uce_delta_kernel(const float* __restrict__ O, const float* __restrict__ N, float* __restrict__ D,
                                                       int m, int ld, const int32_t* __restrict__ row_seg, int P,
                                                       const int32_t* __restrict__ col_seg, int Q, const double* __restrict__ ws) {
    const int p = blockIdx.y, q = blockIdx.x;
    const bool pad = p == P;
    const int r0 = row_seg[p], r1 = pad ? m : row_seg[p + 1];
    const int c0 = col_seg[q], w = col_seg[q + 1] - c0;
    float s = 1.f;
    if (ws && !pad) {
        const double a = ws[2 * ((long)p * Q + q)], b = ws[2 * ((long)p * Q + q) + 1];
        s = (float)(1.0 + (b > 0.0 ? a / b : 0.0));
    }
    const long cnt = (long)(r1 - r0) * w;
    for (long e = threadIdx.x; e < cnt; e += NT) {
        const long r = e / w;
        const long at = (r0 + r) * ld + c0 + (e - r * w);
        D[at] = pad ? 0.f : fmaf(-s, O[at], N[at]);
    }
}

// ---------------------------------------------------------------------------------------------------- debias delta
constexpr int DA = PDMK_DEBIAS_MAX_ATTR;
constexpr int DV = DA + 1;                 // vectors of a block: O, then the attributes
constexpr int DG = DV * (DV + 1) / 2;      // their dot products, (a, b) with a <= b at a DV - a (a - 1) / 2 + b - a

// One workgroup per block (pair p, projection q).  Thread t takes the block's elements t, t + 256, ... in row-major order and
// adds the products of the (A + 1) values there to its (A + 1)(A + 2) / 2 fp64 sums (a product of two fp32 values is exact in
// fp64), then the wave butterfly and the four waves in order, as uce_dot_kernel.  Thread 0 then runs the recurrence
//   c_j = w[p][j] sqrt(t^T G t) / sqrt(G[j + 1][j + 1]),   t = (1, c_0 .. c_{j-1})
// into ws[(p Q + q) A + j]; a zero U_j (the reference: NaN) gives c_j = 0.
__global__ void __launch_bounds__(NT) debias_coef_kernel(const float* __restrict__ O, const float* __restrict__ U, long ustride,
                                                         int ld, int A, const float* __restrict__ w,
                                                         const int32_t* __restrict__ row_seg, const int32_t* __restrict__ col_seg,
                                                         int Q, double* __restrict__ ws) {
    __shared__ double red[DG][NT / 64];
    __shared__ double G[DV][DV];
    __shared__ double t[DV];
    const int p = blockIdx.x / Q, q = blockIdx.x - p * Q;
    const int r0 = row_seg[p], c0 = col_seg[q], wd = col_seg[q + 1] - c0;
    const long cnt = (long)(row_seg[p + 1] - r0) * wd;
    double acc[DG];
#pragma unroll
    for (int g = 0; g < DG; ++g) acc[g] = 0.0;
    for (long e = threadIdx.x; e < cnt; e += NT) {
        const long r = e / wd;
        const long at = (r0 + r) * ld + c0 + (e - r * wd);
        double v[DV];
        v[0] = (double)O[at];
#pragma unroll
        for (int j = 0; j < DA; ++j) v[j + 1] = j < A ? (double)U[j * ustride + at] : 0.0;
#pragma unroll
        for (int a = 0; a < DV; ++a)
#pragma unroll
            for (int b = a; b < DV; ++b)
                if (b <= A) acc[a * DV - a * (a - 1) / 2 + b - a] = fma(v[a], v[b], acc[a * DV - a * (a - 1) / 2 + b - a]);
    }
#pragma unroll
    for (int a = 0; a < DV; ++a)
#pragma unroll
        for (int b = a; b < DV; ++b)
            if (b <= A) {
                const int g = a * DV - a * (a - 1) / 2 + b - a;
                const double s = wave_sum_d(acc[g]);
                if ((threadIdx.x & 63) == 0) red[g][threadIdx.x >> 6] = s;
            }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int a = 0; a <= A; ++a)
            for (int b = a; b <= A; ++b) {
                const int g = a * DV - a * (a - 1) / 2 + b - a;
                G[a][b] = G[b][a] = ((red[g][0] + red[g][1]) + red[g][2]) + red[g][3];
            }
        t[0] = 1.0;
        for (int j = 0; j < A; ++j) {
            double n2 = 0.0;
            for (int a = 0; a <= j; ++a)
                for (int b = 0; b <= j; ++b) n2 = fma(t[a] * t[b], G[a][b], n2);
            const double uu = G[j + 1][j + 1];
            const double c = uu > 0.0 ? (double)w[(long)p * A + j] * sqrt(fmax(n2, 0.0)) / sqrt(uu) : 0.0;
            t[j + 1] = c;
            ws[(long)blockIdx.x * A + j] = c;
        }
    }
}

// grid (Q, P + 1): block (q, p < P) writes D = fp32(sum_j c_j U_j) over its block, the sum in fp64 in the order of j; row
// block P is the padding [row_seg[P], m), written as zeros.  vec: U, D and ld allow 16-byte accesses; a block uses them when
// its first column and width are multiples of 4 as well.
__global__ void __launch_bounds__(NT) debias_delta_kernel(const float* __restrict__ U, long ustride, float* __restrict__ D, int m,
                                                          int ld, int A, const int32_t* __restrict__ row_seg, int P,
                                                          const int32_t* __restrict__ col_seg, int Q, const double* __restrict__ ws,
                                                          int vec) {
    const int p = blockIdx.y, q = blockIdx.x;
    const bool pad = p == P;
    const int r0 = row_seg[p], r1 = pad ? m : row_seg[p + 1];
    const int c0 = col_seg[q], wd = col_seg[q + 1] - c0;
    double c[DA];
#pragma unroll
    for (int j = 0; j < DA; ++j) c[j] = (!pad && j < A) ? ws[((long)p * Q + q) * A + j] : 0.0;
    if (vec && ((c0 | wd) & 3) == 0) {
        const int w4 = wd >> 2;
        const long cnt = (long)(r1 - r0) * w4;
        for (long e = threadIdx.x; e < cnt; e += NT) {
            const long r = e / w4;
            const long at = (r0 + r) * ld + c0 + 4 * (e - r * w4);
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            if (!pad) {
#pragma unroll
                for (int j = 0; j < DA; ++j)
                    if (j < A) {
                        const float4 u = *reinterpret_cast<const float4*>(U + j * ustride + at);
                        s0 = fma(c[j], (double)u.x, s0);
                        s1 = fma(c[j], (double)u.y, s1);
                        s2 = fma(c[j], (double)u.z, s2);
                        s3 = fma(c[j], (double)u.w, s3);
                    }
            }
            *reinterpret_cast<float4*>(D + at) = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
        }
        return;
    }
    const long cnt = (long)(r1 - r0) * wd;
    for (long e = threadIdx.x; e < cnt; e += NT) {
        const long r = e / wd;
        const long at = (r0 + r) * ld + c0 + (e - r * wd);
        double s = 0.0;
        if (!pad) {
#pragma unroll
            for (int j = 0; j < DA; ++j)
                if (j < A) s = fma(c[j], (double)U[j * ustride + at], s);
        }
        D[at] = (float)s;
    }
}

}  // namespace

extern "C" int64_t pdmk_spd_workspace_elems(int n, int m) {
    if (n < 1 || n > PDMK_SPD_MAX_N || m < 1) return 0;
    return ((int64_t)m + RB - 1) / RB * RB * ((n + NB - 1) / NB * NB);
}

extern "C" int pdmk_spd_system_f64(const double* g_a, double s_a, const double* g_b, double s_b, double lam, double* A, int n,
                                   int lda, pdmk_stream s) {
    if (!g_a || !A || n < 1 || n > PDMK_SPD_MAX_N || lda < n || (((uintptr_t)g_a | (uintptr_t)g_b | (uintptr_t)A) & 7)) return -1;
    const long total = (long)n * n;
    const int grid = (int)min(4096L, (total + NT - 1) / NT);
    hipLaunchKernelGGL(spd_system_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)s, g_a, s_a, g_b, s_b, lam, A, n, lda);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_pair_gram_f64(const float* z, int ldz, int npairs, int d, double scale, double lam, double* A, int lda,
                                  pdmk_stream s) {
    if (!z || !A || npairs < 1 || d < 1 || d > PDMK_SPD_MAX_N || ldz < d || lda < d || ((uintptr_t)z & 3) || ((uintptr_t)A & 7))
        return -1;
    const int nt = (d + NB - 1) / NB;
    hipLaunchKernelGGL(pair_gram_kernel, dim3(nt, nt), dim3(NT), 0, (hipStream_t)s, z, ldz, npairs, d, scale, lam, A, lda);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_spd_factor_f64(double* A, int n, int lda, int32_t* info, pdmk_stream s) {
    if (!A || !info || n < 1 || n > PDMK_SPD_MAX_N || lda < n || ((uintptr_t)A & 7) || ((uintptr_t)info & 3)) return -1;
    hipStream_t st = (hipStream_t)s;
    for (int j0 = 0; j0 < n; j0 += NB) {
        hipLaunchKernelGGL(chol_diag_kernel, dim3(1), dim3(NT), 0, st, A, n, lda, j0, info);
        const int below = n - j0 - NB;                        // rows under the diagonal block
        if (below > 0) {
            const int nt = (below + NB - 1) / NB;
            hipLaunchKernelGGL(chol_panel_kernel, dim3((below + NT - 1) / NT), dim3(NT), 0, st, A, n, lda, j0);
            hipLaunchKernelGGL(chol_update_kernel, dim3(nt * (nt + 1) / 2), dim3(NT), 0, st, A, n, lda, j0);
        }
    }
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_spd_solve_f64(const double* L, int n, int ldl, const float* B, int m, int ldb, float* X, int ldx, double* X64,
                                  int ldx64, double* ws, int64_t ws_elems, pdmk_stream s) {
    if (!L || !B || !X || !ws || n < 1 || n > PDMK_SPD_MAX_N || m < 1 || ldl < n || ldb < n || ldx < n || (X64 && ldx64 < n) ||
        (((uintptr_t)L | (uintptr_t)X64 | (uintptr_t)ws) & 7) || (((uintptr_t)B | (uintptr_t)X) & 3) ||
        ws_elems < pdmk_spd_workspace_elems(n, m))
        return -1;
    hipLaunchKernelGGL(spd_solve_kernel, dim3((m + RB - 1) / RB), dim3(NT), 0, (hipStream_t)s, L, n, ldl, B, m, ldb, X, ldx, X64,
                       ldx64, ws);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_uce_delta(const float* O, const float* N, float* D, int m, int ld, const int32_t* row_seg, int P,
                              const int32_t* col_seg, int Q, int technique, double* ws, pdmk_stream s) {
    if (!O || !N || !D || !row_seg || !col_seg || m < 1 || ld < 1 || P < 1 || Q < 1 || P > 65534 || (technique != 0 && technique != 1) ||
        (technique == 1 && (!ws || ((uintptr_t)ws & 7))))
        return -1;
    hipStream_t st = (hipStream_t)s;
    if (technique == 1)
        hipLaunchKernelGGL(uce_dot_kernel, dim3((unsigned)P * (unsigned)Q), dim3(NT), 0, st, O, N, ld, row_seg, col_seg, Q, ws);
    hipLaunchKernelGGL(uce_delta_kernel, dim3(Q, P + 1), dim3(NT), 0, st, O, N, D, m, ld, row_seg, P, col_seg, Q,
                       technique == 1 ? ws : nullptr);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_uce_debias_delta(const float* O, const float* U, float* D, int m, int ld, int A, const float* w,
                                     const int32_t* row_seg, int P, const int32_t* col_seg, int Q, double* ws, int64_t ws_elems,
                                     pdmk_stream s) {
    const uintptr_t words = (uintptr_t)O | (uintptr_t)U | (uintptr_t)D | (uintptr_t)w | (uintptr_t)row_seg | (uintptr_t)col_seg;
    if (!O || !U || !D || !w || !row_seg || !col_seg || !ws || m < 1 || ld < 1 || P < 1 || Q < 1 || P > 65534 || A < 1 ||
        A > PDMK_DEBIAS_MAX_ATTR || (words & 3) || ((uintptr_t)ws & 7) || (int64_t)P * Q > 0x7fffffffLL ||
        ws_elems < (int64_t)P * Q * A)
        return -1;
    hipStream_t st = (hipStream_t)s;
    const long ustride = (long)m * ld;
    const int vec = (ld & 3) == 0 && (((uintptr_t)U | (uintptr_t)D) & 15) == 0;
    hipLaunchKernelGGL(debias_coef_kernel, dim3((unsigned)P * (unsigned)Q), dim3(NT), 0, st, O, U, ustride, ld, A, w, row_seg,
                       col_seg, Q, ws);
    hipLaunchKernelGGL(debias_delta_kernel, dim3(Q, P + 1), dim3(NT), 0, st, U, ustride, D, m, ld, A, row_seg, P, col_seg, Q, ws,
                       vec);
    PDMK_CHECK_LAUNCH();
    return 0;
}
