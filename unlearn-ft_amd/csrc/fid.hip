// Kernels of the FID evaluation (pytorch-fid's InceptionV3 pool3 features + the feature statistics), fp32, inference only.
//   pdmk_conv2d_fwd      : NHWC implicit-GEMM convolution, general (kh, kw, stride, pad_h, pad_w), exact-fp32 MFMA
//                          (v_mfma_f32_16x16x4_f32), fused per-channel bias + ReLU, strided input / output rows so that a
//                          branch of a Mixed block writes its column slice of the block's output buffer (no concat copy).
//   pdmk_conv2d_fwd_res  : the same launch with a residual operand (fp32, laid out like the output) added between the bias and
//                          the ReLU in the epilogue: ResNet's relu(bn(conv3) + identity).  The K loop is untouched.
//   pdmk_pool2d          : NHWC 3x3 max pool and 3x3 average pool whose divisor is the number of taps inside the image
//                          (count_include_pad=False), any stride / pad <= 1.
//   pdmk_global_avgpool  : [B, HW, C] -> [B, C], one thread per output, rows summed in order.
//   pdmk_fid_accumulate  : sum[D] += sum_r x[r], outer[D, D] += sum_r x[r] x[r]^T (upper-triangle tiles) in fp64; each output
//                          tile is owned by one workgroup that walks the rows in order: no atomics, bit-reproducible.
//
// Convolution: C[m][n] = sum_k A[m][k] W[n][k], m = (b, oy, ox), k = (ky, kx, ci), A gathered from the image on the fly (taps
// outside the image are zero; there is no im2col matrix in memory).  One workgroup of 4 waves per 128 x 64 output tile (64 x 64 where the
// larger tile would give fewer than two workgroups per CU), K in
// steps of 16: the next step's operands are fetched from global memory into registers while the MFMAs of the current step
// read LDS.  Both operand tiles sit in LDS reduction-major ([k][m], [k][n]) so that a fragment read (lane l: row l & 15 at
// k = l >> 4) touches 16 consecutive words per k.  Wave w owns rows 32w .. 32w+31 (16w .. 16w+15) of the tile and all 64 columns:
// 2 x 4 (1 x 4) MFMA tiles.  With Ci % 4 == 0 (every unit but the first, Ci = 3) four consecutive k share a tap and are one
// aligned 16-byte load; otherwise every element is gathered on its own.  Tails in M, Co and K are zero-filled on the way into
// LDS and masked on the way out.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int BN = 64, BK = 16;      // the tile is 64 WM x 64 (WM = 2, or 1 where 128-row tiles would leave CUs idle)
// LDS row strides (words), both 8 mod 32: the four k of a fragment read (lanes 16 g .. 16 g + 15 at k + g) start 8 banks apart,
// so every bank serves exactly two lanes - the floor for 64 lanes.  The staging writes (lane: k chunk l & 3, row l >> 2) would
// put the four chunks on the same banks; each lane therefore writes its four values in an order rotated by its chunk number.
constexpr int RSB = BN + 8;

struct ConvGeom {
    int B, H, W, Ci, Co, kh, kw, stride, ph, pw, Ho, Wo, lda, ldc, M, K, relu, ldr;
};

template <bool VEC, int WM>
__global__ __launch_bounds__(NT) void conv2d_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                    const float* __restrict__ bias, const float* res, float* y, ConvGeom g) {
    constexpr int BM = 64 * WM, RSA = BM + 8;
    __shared__ float As[BK * RSA];
    __shared__ float Bs[BK * RSB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

    // staging roles.  VEC: thread -> (k chunk kc = tid & 3, row tid >> 2 [+ 64]) of A, (kc, column tid >> 2) of B.
    // scalar: thread -> k = tid & 15, rows (tid >> 4) + 16 i of A (4 WM of them), columns (tid >> 4) + 16 i of B (4).
    constexpr int NA = VEC ? WM : 4 * WM, NB = VEC ? 1 : 4;
    const int kk = VEC ? (tid & 3) * 4 : (tid & 15);
    long abase[NA];            // element offset of (b, iy0, ix0, 0) of the row's window; only used where the tap is inside
    int aiy[NA], aix[NA];      // iy0, ix0 (may be negative); row beyond M: iy0 = a large negative number (never inside)
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int r = VEC ? (tid >> 2) + 64 * i : (tid >> 4) + 16 * i;
        const int m = m0 + r;
        if (m < g.M) {
            const int b = m / (g.Ho * g.Wo), p = m - b * g.Ho * g.Wo;
            const int oy = p / g.Wo, ox = p - oy * g.Wo;
            aiy[i] = oy * g.stride - g.ph;
            aix[i] = ox * g.stride - g.pw;
            abase[i] = (((long)b * g.H + aiy[i]) * g.W + aix[i]) * g.lda;
        } else {
            aiy[i] = -(1 << 28);
            aix[i] = 0;
            abase[i] = 0;
        }
    }

    float4 ra[VEC ? NA : 1], rb[VEC ? NB : 1];
    float sa[VEC ? 1 : NA], sb[VEC ? 1 : NB];

    auto fetch = [&](int k0) {
        const int k = k0 + kk;
        int ky = 0, kx = 0, ci = 0;
        const bool kin = k < g.K;
        if (kin) {
            const int tap = k / g.Ci;
            ci = k - tap * g.Ci;
            ky = tap / g.kw;
            kx = tap - ky * g.kw;
        }
        const long koff = ((long)ky * g.W + kx) * g.lda + ci;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int iy = aiy[i] + ky, ix = aix[i] + kx;
            const bool in = kin && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
            if constexpr (VEC) {
                ra[i] = in ? *reinterpret_cast<const float4*>(x + abase[i] + koff) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                sa[i] = in ? x[abase[i] + koff] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int n = n0 + (VEC ? (tid >> 2) : (tid >> 4) + 16 * i);
            const bool in = kin && n < g.Co;
            if constexpr (VEC) {
                rb[i] = in ? *reinterpret_cast<const float4*>(w + (long)n * g.K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                sb[i] = in ? w[(long)n * g.K + k] : 0.f;
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            if constexpr (VEC) {
                const int r = (tid >> 2) + 64 * i;
                const float v[4] = {ra[i].x, ra[i].y, ra[i].z, ra[i].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int jj = (j + (tid & 3)) & 3;
                    As[(kk + jj) * RSA + r] = jj == 0 ? v[0] : jj == 1 ? v[1] : jj == 2 ? v[2] : v[3];
                }
            } else {
                As[kk * RSA + (tid >> 4) + 16 * i] = sa[i];
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if constexpr (VEC) {
                const int c = tid >> 2;
                const float v[4] = {rb[i].x, rb[i].y, rb[i].z, rb[i].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int jj = (j + (tid & 3)) & 3;
                    Bs[(kk + jj) * RSB + c] = jj == 0 ? v[0] : jj == 1 ? v[1] : jj == 2 ? v[2] : v[3];
                }
            } else {
                Bs[kk * RSB + (tid >> 4) + 16 * i] = sb[i];
            }
        }
    };

    f32x4 acc[WM][4];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    fetch(0);
    for (int k0 = 0; k0 < g.K; k0 += BK) {
        __syncthreads();                      // the previous step's fragment reads are done
        stage();
        __syncthreads();
        if (k0 + BK < g.K) fetch(k0 + BK);    // in flight while the MFMAs below run
#pragma unroll
        for (int ks = 0; ks < BK; ks += 4) {
            float a[WM], b[4];
#pragma unroll
            for (int i = 0; i < WM; ++i) a[i] = Mma<float>::load_colk(As, RSA, ks, wave * 16 * WM + 16 * i, lane);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Mma<float>::load_colk(Bs, RSB, ks, 16 * j, lane);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = Mma<float>::mma(a[i], b[j], acc[i][j]);
        }
    }

    // epilogue: lane l holds rows 4 (l >> 4) + r, column l & 15 of each 16 x 16 tile.  res may be y itself (neither is
    // __restrict__): a thread reads its elements of res before it writes those elements of y, and no other thread touches
    // them.  The residual values of a column tile are fetched together before that tile is stored: four round trips, not one
    // per element behind a store it could alias.  (Fetching the whole fragment, or one tile ahead, costs the 128-row form
    // a wave of occupancy, with or without a residual.)
    float rv[WM][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (res) {
            const int nr = n0 + 16 * j + (lane & 15);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + wave * 16 * WM + 16 * i + 4 * (lane >> 4) + r;
                    rv[i][r] = (nr < g.Co && m < g.M) ? res[(long)m * g.ldr + nr] : 0.f;
                }
        }
        const int n = n0 + 16 * j + (lane & 15);
        if (n >= g.Co) continue;
        const float bv = bias ? bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wave * 16 * WM + 16 * i + 4 * (lane >> 4) + r;
                if (m < g.M) {
                    float v = acc[i][j][r] + bv;
                    if (res) v += rv[i][r];
                    if (g.relu) v = fmaxf(v, 0.f);
                    y[(long)m * g.ldc + n] = v;
                }
            }
    }
}

// ---- pools.  One thread per output element, channel fastest (coalesced rows).  The taps are visited in (ky, kx) order.
template <bool AVG>
__global__ __launch_bounds__(NT) void pool3x3_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, int B,
                                                     int H, int W, int C, int stride, int pad, int Ho, int Wo) {
    const long n = (long)B * Ho * Wo * C;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const long pix = i / C;
        const int c = (int)(i - pix * C);
        const int b = (int)(pix / (Ho * Wo)), p = (int)(pix - (long)b * Ho * Wo);
        const int oy = p / Wo, ox = p - oy * Wo;
        float acc = AVG ? 0.f : -INFINITY;
        int cnt = 0;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * stride - pad + ky;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * stride - pad + kx;
                if (ix < 0 || ix >= W) continue;
                const float v = x[(((long)b * H + iy) * W + ix) * ldx + c];
                if (AVG) acc += v;
                else acc = (v > acc || v != v) ? v : acc;      // NaN propagates, as torch's max pool does
                ++cnt;
            }
        }
        y[pix * ldy + c] = AVG ? acc / (float)cnt : acc;
    }
}

__global__ __launch_bounds__(NT) void global_avgpool_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int B,
                                                            int HW, int C) {
    const long n = (long)B * C;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const long b = i / C;
        const int c = (int)(i - b * C);
        const float* p = x + b * HW * ldx + c;
        float s = 0.f;
        for (int r = 0; r < HW; ++r) s += p[(long)r * ldx];
        y[i] = s / (float)HW;
    }
}

// ---- statistics.  Tile (ti, tj), ti <= tj, of the 64 x 64 tiling of outer[D][D]; thread (ty, tx) of 16 x 16 owns the 4 x 4
// block rows 4 ty .., columns tx + 16 c (columns interleaved: conflict-free LDS reads, 128-byte store segments).
constexpr int FT = 64, FR = 16;     // tile side, rows staged per step
__global__ __launch_bounds__(NT) void fid_accumulate_kernel(const float* __restrict__ x, int ldx, int B, int D,
                                                            double* __restrict__ sum, double* __restrict__ outer) {
    __shared__ float xi[FR][FT], xj[FR][FT];
    // linear id -> (ti, tj) of the upper triangle, row by row
    const int nt = (D + FT - 1) / FT;
    int ti = 0, rem = blockIdx.x;
    while (rem >= nt - ti) {
        rem -= nt - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const int i0 = ti * FT, j0 = tj * FT;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;

    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + 4 * ty + a, j = j0 + tx + 16 * c;
            acc[a][c] = (i < D && j < D) ? outer[(long)i * D + j] : 0.0;
        }
    const bool do_sum = ti == tj && threadIdx.x < FT && i0 + (int)threadIdx.x < D;
    double s = do_sum ? sum[i0 + threadIdx.x] : 0.0;

    for (int r0 = 0; r0 < B; r0 += FR) {
        __syncthreads();
        for (int e = threadIdx.x; e < FR * FT; e += NT) {
            const int r = e / FT, c = e - r * FT;
            const bool rin = r0 + r < B;
            xi[r][c] = (rin && i0 + c < D) ? x[(long)(r0 + r) * ldx + i0 + c] : 0.f;
            xj[r][c] = (rin && j0 + c < D) ? x[(long)(r0 + r) * ldx + j0 + c] : 0.f;
        }
        __syncthreads();
        const int nr = B - r0 < FR ? B - r0 : FR;
        for (int r = 0; r < nr; ++r) {
            double u[4], v[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) u[a] = (double)xi[r][4 * ty + a];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = (double)xj[r][tx + 16 * c];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] = fma(u[a], v[c], acc[a][c]);
            if (do_sum) s += (double)xi[r][threadIdx.x];
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + 4 * ty + a, j = j0 + tx + 16 * c;
            if (i < D && j < D) outer[(long)i * D + j] = acc[a][c];
        }
    if (do_sum) sum[i0 + threadIdx.x] = s;
}

unsigned grid_for(long n) {
    const long g = (n + NT - 1) / NT;
    return (unsigned)(g < 16384 ? g : 16384);
}

}  // namespace

extern "C" int pdmk_conv2d_fwd_res(const float* x, int lda, const float* w, const float* bias, const float* res, int ldr, float* y,
                                   int ldc, int B, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad_h, int pad_w,
                                   int relu, pdmk_stream stream) {
    if (res && (ldr < Co || ((uintptr_t)res & 3))) return -1;
    if (!x || !w || !y || B < 1 || H < 1 || W < 1 || Ci < 1 || Co < 1 || kh < 1 || kw < 1 || kh > 16 || kw > 16 || stride < 1 ||
        pad_h < 0 || pad_w < 0 || pad_h >= kh || pad_w >= kw || lda < Ci || ldc < Co || H + 2 * pad_h < kh || W + 2 * pad_w < kw)
        return -1;
    ConvGeom g;
    g.B = B, g.H = H, g.W = W, g.Ci = Ci, g.Co = Co, g.kh = kh, g.kw = kw, g.stride = stride, g.ph = pad_h, g.pw = pad_w;
    g.Ho = (H + 2 * pad_h - kh) / stride + 1;
    g.Wo = (W + 2 * pad_w - kw) / stride + 1;
    g.lda = lda, g.ldc = ldc, g.relu = relu ? 1 : 0, g.ldr = res ? ldr : 0;
    const int64_t M = (int64_t)B * g.Ho * g.Wo, K = (int64_t)kh * kw * Ci;
    if (M > (1ll << 30) || K > (1ll << 24) || (int64_t)B * H * W * lda > (1ll << 40)) return -1;
    g.M = (int)M, g.K = (int)K;
    const int64_t gy = (Co + BN - 1) / BN;
    if (gy > 65535) return -1;
    const bool vec = Ci % 4 == 0 && lda % 4 == 0 && !((uintptr_t)x & 15) && !((uintptr_t)w & 15);
    // 128-row tiles unless they give fewer than two workgroups per CU (256 CUs): the 8 x 8 and 17 x 17 maps at small batches
    const bool small = (M + 127) / 128 * gy < 512;
    dim3 grid((unsigned)((M + (small ? 63 : 127)) / (small ? 64 : 128)), (unsigned)gy);
    hipStream_t st = (hipStream_t)stream;
    if (vec && small) hipLaunchKernelGGL((conv2d_kernel<true, 1>), grid, dim3(NT), 0, st, x, w, bias, res, y, g);
    else if (vec) hipLaunchKernelGGL((conv2d_kernel<true, 2>), grid, dim3(NT), 0, st, x, w, bias, res, y, g);
    else if (small) hipLaunchKernelGGL((conv2d_kernel<false, 1>), grid, dim3(NT), 0, st, x, w, bias, res, y, g);
    else hipLaunchKernelGGL((conv2d_kernel<false, 2>), grid, dim3(NT), 0, st, x, w, bias, res, y, g);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_conv2d_fwd(const float* x, int lda, const float* w, const float* bias, float* y, int ldc, int B, int H, int W,
                               int Ci, int Co, int kh, int kw, int stride, int pad_h, int pad_w, int relu, pdmk_stream stream) {
    return pdmk_conv2d_fwd_res(x, lda, w, bias, nullptr, 0, y, ldc, B, H, W, Ci, Co, kh, kw, stride, pad_h, pad_w, relu, stream);
}

extern "C" int pdmk_pool2d(const float* x, int ldx, float* y, int ldy, int B, int H, int W, int C, int mode, int stride, int pad,
                           pdmk_stream stream) {
    if (!x || !y || B < 1 || H < 1 || W < 1 || C < 1 || ldx < C || ldy < C || (mode != 0 && mode != 1) || stride < 1 || pad < 0 ||
        pad > 1 || H + 2 * pad < 3 || W + 2 * pad < 3 || (int64_t)B * H * W * ldx > (1ll << 40))
        return -1;
    const int Ho = (H + 2 * pad - 3) / stride + 1, Wo = (W + 2 * pad - 3) / stride + 1;
    const long n = (long)B * Ho * Wo * C;
    if (mode) hipLaunchKernelGGL(pool3x3_kernel<true>, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, x, ldx, y, ldy, B, H, W, C, stride, pad, Ho, Wo);
    else hipLaunchKernelGGL(pool3x3_kernel<false>, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, x, ldx, y, ldy, B, H, W, C, stride, pad, Ho, Wo);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_global_avgpool(const float* x, int ldx, float* y, int B, int HW, int C, pdmk_stream stream) {
    if (!x || !y || B < 1 || HW < 1 || C < 1 || ldx < C) return -1;
    hipLaunchKernelGGL(global_avgpool_kernel, dim3(grid_for((long)B * C)), dim3(NT), 0, (hipStream_t)stream, x, ldx, y, B, HW, C);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_fid_accumulate(const float* x, int ldx, int B, int D, double* sum, double* outer, pdmk_stream stream) {
    if (!x || !sum || !outer || B < 1 || D < 1 || D > (1 << 15) || ldx < D || ((uintptr_t)sum & 7) || ((uintptr_t)outer & 7)) return -1;
    const int nt = (D + FT - 1) / FT;
    hipLaunchKernelGGL(fid_accumulate_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(NT), 0, (hipStream_t)stream, x, ldx, B, D,
                       sum, outer);
    PDMK_CHECK_LAUNCH();
    return 0;
}
