// Kernels of the perceptual metrics of the erasure evaluation (pdm/utils/perceptual.py): LPIPS (AlexNet) and the VGG-19
// Gram-matrix style loss / content loss.  fp32 NHWC maps [B, HW, ld] (ld >= C: a map may be a column slice), inference only,
// no float atomics anywhere: the same arguments give the same bits on every launch.
//   pdmk_relu_pool   : y = max(x, 0), optionally followed by a 2 x 2 stride-2 max pool with floor sizes.  The VGG trunk taps its
//                      convolutions BEFORE the ReLU, so those convs run without the fused ReLU and this kernel feeds the next one.
//   pdmk_lpips_layer : one layer of LPIPS v0.1: unit-normalise both feature vectors of a pixel (eps added to the norm), weighted
//                      squared difference over the channels, mean over the pixels, added to out[b] in fp64.  A 16-lane group per
//                      pixel; the two norms and the weighted sum are shuffle reductions in registers; 16-byte loads where the
//                      slice allows them.  One workgroup per image walks its pixels in a fixed order.
//   pdmk_gram_pair   : G_i = X_i^T X_i / (C HW) of both maps of a pair, style += mean((G_0 - G_1)^2), content += mean((f0 - f1)^2)
//                      in one pass over the two maps.  X is tall and skinny (HW up to 2^18, C = 64 .. 256) and the pass is
//                      bandwidth-bound, so HW is split over workgroups: workgroup (tile, split, image) accumulates the 64 x 64
//                      tile (ti <= tj) of both Gram matrices over its rows on the exact-fp32 MFMA (Mma<float>, common.h), 32 rows
//                      per fp32 chain and fp64 across the chains, and writes the two partial tiles to the workspace; the finish pass adds the partials of a tile in split order,
//                      scales each G in fp32, squares the difference in fp64 (tiles above the diagonal count twice: X^T X is
//                      symmetric bit for bit, the products commute and the k order is the same); a last launch adds the per-tile
//                      sums in order.  Rows are read [k][column], which is the layout in memory: both MFMA operands are
//                      reduction-major LDS images read with load_colk, no transpose anywhere.  The diagonal tiles take the
//                      content loss from the registers they stage.
#include "common.h"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ float relu_nan(float v) { return v > 0.f ? v : (v != v ? v : 0.f); }      // NaN stays, as torch.relu
__device__ __forceinline__ float max_nan(float a, float v) { return (v > a || v != v) ? v : a; }      // as pool3x3_kernel (fid.hip)

// no __restrict__: with pool 0 the caller may pass y == x (every thread reads and writes its own element only)
__global__ __launch_bounds__(NT) void relu_pool_kernel(const float* x, int ldx, float* y, int ldy, int B, int H, int W, int C,
                                                       int pool, int Ho, int Wo) {
    const long n = (long)B * Ho * Wo * C;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const long pix = i / C;
        const int c = (int)(i - pix * C);
        if (!pool) {
            y[pix * ldy + c] = relu_nan(x[pix * ldx + c]);
            continue;
        }
        const int b = (int)(pix / (Ho * Wo)), p = (int)(pix - (long)b * Ho * Wo);
        const int oy = p / Wo, ox = p - oy * Wo;
        const float* q = x + (((long)b * H + 2 * oy) * W + 2 * ox) * ldx + c;          // 2 oy + 1 < H, 2 ox + 1 < W (floor sizes)
        float m = relu_nan(q[0]);
        m = max_nan(m, relu_nan(q[ldx]));
        m = max_nan(m, relu_nan(q[(long)W * ldx]));
        m = max_nan(m, relu_nan(q[(long)(W + 1) * ldx]));
        y[pix * ldy + c] = m;
    }
}

// ---- LPIPS layer.  Group g (16 lanes) of the workgroup takes pixels g, g + 16, ...; lane j of it the channels 4 j + 64 i (VEC)
// or j + 16 i.  Two sweeps over the pixel's two rows: the squared norms, then the weighted difference (the second sweep hits L1).
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(NT) void lpips_layer_kernel(const float* __restrict__ f0, const float* __restrict__ f1, int ld,
                                                         const float* __restrict__ w, double* __restrict__ out, int HW, int C) {
    __shared__ double red[NT / 16];
    const int b = blockIdx.x, grp = threadIdx.x >> 4, j = threadIdx.x & 15;
    const float* x0 = f0 + (long)b * HW * ld;
    const float* x1 = f1 + (long)b * HW * ld;
    double acc = 0.0;
    for (int p = grp; p < HW; p += NT / 16) {
        const float* r0 = x0 + (long)p * ld;
        const float* r1 = x1 + (long)p * ld;
        float s0 = 0.f, s1 = 0.f;
        if constexpr (VEC) {
            for (int c = 4 * j; c < C; c += 64) {
                const float4 a = *reinterpret_cast<const float4*>(r0 + c), e = *reinterpret_cast<const float4*>(r1 + c);
                s0 += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
                s1 += e.x * e.x + e.y * e.y + e.z * e.z + e.w * e.w;
            }
        } else {
            for (int c = j; c < C; c += 16) {
                s0 += r0[c] * r0[c];
                s1 += r1[c] * r1[c];
            }
        }
        const float d0 = sqrtf(group16_sum(s0)) + 1e-10f, d1 = sqrtf(group16_sum(s1)) + 1e-10f;
        float t = 0.f;
        if constexpr (VEC) {
            for (int c = 4 * j; c < C; c += 64) {
                const float4 a = *reinterpret_cast<const float4*>(r0 + c), e = *reinterpret_cast<const float4*>(r1 + c);
                const float4 k = *reinterpret_cast<const float4*>(w + c);
                const float ux = a.x / d0 - e.x / d1, uy = a.y / d0 - e.y / d1, uz = a.z / d0 - e.z / d1, uw = a.w / d0 - e.w / d1;
                t += k.x * (ux * ux) + k.y * (uy * uy) + k.z * (uz * uz) + k.w * (uw * uw);
            }
        } else {
            for (int c = j; c < C; c += 16) {
                const float u = r0[c] / d0 - r1[c] / d1;
                t += w[c] * (u * u);
            }
        }
        acc += (double)group16_sum(t);            // every lane of the group holds the pixel's value; lane 0's copy is used below
    }
    if (j == 0) red[grp] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int g = 0; g < NT / 16; ++g) s += red[g];
        out[b] += s / (double)HW;
    }
}

// ---- Gram pair
constexpr int GT = 64, GK = 32, GRS = GT + 8;       // tile side, rows per step, LDS row stride (8 mod 32: see fid.hip)
constexpr int GSL = GT * GT / NT;                   // slices of a tile in the finish pass (one element per thread each)
constexpr int GWANT = 1024, GMINROWS = 512;         // workgroups aimed at (4 per CU), fewest rows per split

struct GramPlan {
    int nt, T, S, chunk;
    int64_t o_content, o_style, total;              // offsets / size in floats
};

bool gram_plan(int B, int HW, int C, GramPlan& p) {
    if (B < 1 || HW < 1 || C < 1 || C > 2048 || B > 65535) return false;
    p.nt = (C + GT - 1) / GT;
    p.T = p.nt * (p.nt + 1) / 2;
    const int64_t tb = (int64_t)p.T * B;
    int64_t want = (GWANT + tb - 1) / tb;
    if (want < 1) want = 1;
    int64_t chunk = (HW + want - 1) / want;
    if (chunk < GMINROWS) chunk = GMINROWS;
    chunk = (chunk + GK - 1) / GK * GK;
    p.chunk = (int)chunk;
    p.S = (int)((HW + chunk - 1) / chunk);
    if ((int64_t)p.T * p.S > (1ll << 30)) return false;
    p.o_content = (int64_t)B * p.S * p.T * 2 * GT * GT;
    p.o_style = p.o_content + 2ll * B * p.S * p.nt;
    p.total = p.o_style + 2ll * B * p.T * GSL;
    return true;
}

__device__ __forceinline__ void tile_of(int t, int nt, int& ti, int& tj) {     // linear id -> (ti, tj), ti <= tj, row by row
    ti = 0;
    while (t >= nt - ti) {
        t -= nt - ti;
        ++ti;
    }
    tj = ti + t;
}

template <bool VEC>
__global__ __launch_bounds__(NT) void gram_partial_kernel(const float* __restrict__ f0, const float* __restrict__ f1, int ld,
                                                          int HW, int C, int nt, int T, int S, int chunk,
                                                          float* __restrict__ part, double* __restrict__ cpart) {
    __shared__ __attribute__((aligned(16))) float P[2][2][GK * GRS];      // [map][panel i / j][k][column]
    __shared__ double red[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x % T, s = blockIdx.x / T, b = blockIdx.y;
    int ti, tj;
    tile_of(t, nt, ti, tj);
    const bool diag = ti == tj;
    const int np = diag ? 1 : 2;
    const float* xs[2] = {f0 + (long)b * HW * ld, f1 + (long)b * HW * ld};
    const int rbeg = s * chunk, rend = min(HW, rbeg + chunk);
    const int kr = tid >> 4, c4 = (tid & 15) * 4;                           // staging role: rows kr, kr + 16 of the step, 4 columns

    float4 reg[2][2][2];                                                    // [map][panel][row half]
    auto fetch = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = k0 + kr + 16 * h;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                if (p >= np) continue;
                const int col = (p ? tj : ti) * GT + c4;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (row < rend) {
                        const float* q = xs[m] + (long)row * ld + col;
                        if constexpr (VEC) {
                            if (col < C) v = *reinterpret_cast<const float4*>(q);
                        } else {
                            if (col < C) v.x = q[0];
                            if (col + 1 < C) v.y = q[1];
                            if (col + 2 < C) v.z = q[2];
                            if (col + 3 < C) v.w = q[3];
                        }
                    }
                    reg[m][p][h] = v;
                }
            }
        }
    };

    f32x4 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // second level of the row sum: each step's 32-row fp32 MFMA chain is added to fp64 accumulators, so the rounding error of a
    // Gram entry does not grow with the rows of the split (a 512-row fp32 chain loses ~4 x more, and the style loss takes the
    // DIFFERENCE of two such matrices)
    double dacc[2][4][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) dacc[m][j][r] = 0.0;
    double cs = 0.0;

    fetch(rbeg);
    for (int k0 = rbeg; k0 < rend; k0 += GK) {
        __syncthreads();                      // the previous step's fragment reads are done
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                if (p >= np) continue;
#pragma unroll
                for (int m = 0; m < 2; ++m)
                    *reinterpret_cast<float4*>(&P[m][p][(kr + 16 * h) * GRS + c4]) = reg[m][p][h];
            }
            if (diag) {                       // content loss of this tile's 64 columns (rows / columns outside the map are 0 - 0)
                const float4 a = reg[0][0][h], e = reg[1][0][h];
                const float dx = a.x - e.x, dy = a.y - e.y, dz = a.z - e.z, dw = a.w - e.w;
                cs += (double)(dx * dx + dy * dy + dz * dz + dw * dw);
            }
        }
        __syncthreads();
        if (k0 + GK < rend) fetch(k0 + GK);   // in flight while the MFMAs below run
        const int pj = diag ? 0 : 1;
#pragma unroll
        for (int ks = 0; ks < GK; ks += 4) {
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const float a = Mma<float>::load_colk(P[m][0], GRS, ks, 16 * wave, lane);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[m][j] = Mma<float>::mma(a, Mma<float>::load_colk(P[m][pj], GRS, ks, 16 * j, lane), acc[m][j]);
            }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) dacc[m][j][r] += (double)acc[m][j][r];
                acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
    }

    // partial tiles: lane l holds rows 16 wave + 4 (l >> 4) + r, column 16 j + (l & 15)
    float* dst = part + (((long)b * S + s) * T + t) * 2 * GT * GT;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                dst[m * GT * GT + (16 * wave + 4 * (lane >> 4) + r) * GT + 16 * j + (lane & 15)] = (float)dacc[m][j][r];
    if (diag) {
        cs = wave_sum_d(cs);
        if (lane == 0) red[wave] = cs;
        __syncthreads();
        if (tid == 0) cpart[((long)b * S + s) * nt + ti] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// slice (256 elements) of tile t of image b: partials added in split order (fp64, rounded once to fp32: the Gram entry as one
// fp32 number), each G divided in fp32, the squared difference in fp64
__global__ __launch_bounds__(NT) void gram_finish_kernel(const float* __restrict__ part, int nt, int T, int S, int C, float denom,
                                                         double* __restrict__ spart) {
    __shared__ double red[NT / 64];
    const int t = blockIdx.x / GSL, slice = blockIdx.x % GSL, b = blockIdx.y;
    int ti, tj;
    tile_of(t, nt, ti, tj);
    const int e = slice * NT + threadIdx.x;
    const int i = ti * GT + (e >> 6), j = tj * GT + (e & 63);
    double s0 = 0.0, s1 = 0.0;
    for (int s = 0; s < S; ++s) {
        const float* src = part + (((long)b * S + s) * T + t) * 2 * GT * GT + e;
        s0 += (double)src[0];
        s1 += (double)src[GT * GT];
    }
    const float d = (float)s0 / denom - (float)s1 / denom;
    double v = (i < C && j < C) ? (double)d * (double)d : 0.0;
    if (ti != tj) v *= 2.0;
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) spart[((long)b * T + t) * GSL + slice] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void gram_total_kernel(const double* __restrict__ spart, const double* __restrict__ cpart, int nt, int T, int S, int HW,
                                  int C, double* __restrict__ style_out, double* __restrict__ content_out) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    double st = 0.0;
    for (int i = 0; i < T * GSL; ++i) st += spart[(long)b * T * GSL + i];
    style_out[b] += st / ((double)C * (double)C);
    if (content_out) {
        double ct = 0.0;
        for (int i = 0; i < S * nt; ++i) ct += cpart[(long)b * S * nt + i];
        content_out[b] += ct / ((double)HW * (double)C);
    }
}

unsigned grid_for(long n) {
    const long g = (n + NT - 1) / NT;
    return (unsigned)(g < 16384 ? g : 16384);
}

bool vec_ok(const void* a, const void* b, int ld, int C) {
    return C % 4 == 0 && ld % 4 == 0 && !((uintptr_t)a & 15) && !((uintptr_t)b & 15);
}

}  // namespace

extern "C" int pdmk_relu_pool(const float* x, int ldx, float* y, int ldy, int B, int H, int W, int C, int pool, pdmk_stream stream) {
    if (!x || !y || ((uintptr_t)x & 3) || ((uintptr_t)y & 3) || B < 1 || H < 1 || W < 1 || C < 1 || ldx < C || ldy < C ||
        (pool != 0 && pool != 2) || (int64_t)B * H * W * ldx > (1ll << 40) || (int64_t)B * H * W * ldy > (1ll << 40))
        return -1;
    const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
    if (Ho < 1 || Wo < 1) return -1;
    hipLaunchKernelGGL(relu_pool_kernel, dim3(grid_for((long)B * Ho * Wo * C)), dim3(NT), 0, (hipStream_t)stream, x, ldx, y, ldy, B,
                       H, W, C, pool, Ho, Wo);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_lpips_layer(const float* f0, const float* f1, int ld, const float* w, double* out, int B, int HW, int C,
                                pdmk_stream stream) {
    if (!f0 || !f1 || !w || !out || ((uintptr_t)f0 & 3) || ((uintptr_t)f1 & 3) || ((uintptr_t)w & 3) || ((uintptr_t)out & 7) ||
        B < 1 || HW < 1 || C < 1 || ld < C || (int64_t)B * HW * ld > (1ll << 40))
        return -1;
    if (vec_ok(f0, f1, ld, C) && !((uintptr_t)w & 15))
        hipLaunchKernelGGL(lpips_layer_kernel<true>, dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream, f0, f1, ld, w, out, HW, C);
    else
        hipLaunchKernelGGL(lpips_layer_kernel<false>, dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream, f0, f1, ld, w, out, HW, C);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t pdmk_gram_workspace_elems(int B, int HW, int C) {
    GramPlan p;
    return gram_plan(B, HW, C, p) ? p.total : -1;
}

extern "C" int pdmk_gram_pair(const float* f0, const float* f1, int ld, int B, int HW, int C, float* ws, int64_t ws_elems,
                              double* style_out, double* content_out, pdmk_stream stream) {
    GramPlan p;
    if (!f0 || !f1 || !ws || !style_out || ((uintptr_t)f0 & 3) || ((uintptr_t)f1 & 3) || ((uintptr_t)ws & 15) ||
        ((uintptr_t)style_out & 7) || ((uintptr_t)content_out & 7) || !gram_plan(B, HW, C, p) || ld < C || ws_elems < p.total ||
        (int64_t)B * HW * ld > (1ll << 40) || (int64_t)HW * C > (1ll << 40))
        return -1;
    hipStream_t st = (hipStream_t)stream;
    double* cpart = reinterpret_cast<double*>(ws + p.o_content);
    double* spart = reinterpret_cast<double*>(ws + p.o_style);
    const dim3 grid((unsigned)(p.T * p.S), (unsigned)B);
    if (vec_ok(f0, f1, ld, C))
        hipLaunchKernelGGL(gram_partial_kernel<true>, grid, dim3(NT), 0, st, f0, f1, ld, HW, C, p.nt, p.T, p.S, p.chunk, ws, cpart);
    else
        hipLaunchKernelGGL(gram_partial_kernel<false>, grid, dim3(NT), 0, st, f0, f1, ld, HW, C, p.nt, p.T, p.S, p.chunk, ws, cpart);
    PDMK_CHECK_LAUNCH();
    hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)(p.T * GSL), (unsigned)B), dim3(NT), 0, st, ws, p.nt, p.T, p.S, C,
                       (float)((double)C * (double)HW), spart);
    PDMK_CHECK_LAUNCH();
    hipLaunchKernelGGL(gram_total_kernel, dim3((unsigned)B), dim3(64), 0, st, spart, cpart, p.nt, p.T, p.S, HW, C, style_out,
                       content_out);
    PDMK_CHECK_LAUNCH();
    return 0;
}
