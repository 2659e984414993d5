// Sampler kernels (include/pdmk.h "Sampler"): the fused guidance + PLMS step between two U-Net calls of the denoising loop,
// and the uint8 image epilogue of the FID image generator.
//
// pdmk_plms_step reproduces, bit for bit, the eager chain of StableDiffusionPruningPipeline.generate_samples:
//   nhwc_to_nchw of the prediction (exact: bf16 -> fp32 is exact) -> guidance axpby -> PNDMScheduler.step's clone / axpby
//   chain -> the next call's two latent copies and nchw_to_nhwc.
// pdmk_ddim_step is the same launch for DDIMScheduler.step (one axpby: prev = c_m * model_output + c_x * sample).
// Every fp32 combination is pdmk_axpby's: ew_kernel<float, 2> computes `alpha * f + beta * o`, which the Makefile's default
// contraction turns into `v_pk_mul_f32 (beta * o)` + `v_pk_fma_f32 (alpha, f, that)` on its 16-byte path (the one every
// latent-sized call takes: B * 4 * H * W is a multiple of 4).  form() below spells that out as fma(a, x, b * y), and this file
// is compiled without contraction so that nothing else is fused.  fp32 -> bf16 of the next U-Net input is from_f32<bf16>, as
// in nchw2nhwc_kernel.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
inline int grid_for(long nwork, int cap = 1024) { return (int)max(1L, min((long)cap, (nwork + NT - 1) / NT)); }

__device__ __forceinline__ float form(float a, float x, float b, float y) { return __builtin_fmaf(a, x, b * y); }

template <typename T>
__global__ void plms_step_kernel(const T* __restrict__ pred, int ld, float g_u, float g_t, int cfg,
                                 float* __restrict__ sample, float* __restrict__ cur, float* __restrict__ ets,
                                 const pdmk_plms_row* __restrict__ table, int nsteps, int32_t* state,
                                 int64_t* __restrict__ t_out, T* __restrict__ x_next, int cpad, int B, int C, int HW) {
    const int step = state[0];
    if (step < 0 || step >= nsteps) return;          // every workgroup reads the same counter: all of them return
    const pdmk_plms_row& r = table[step];
    const long N = (long)B * C * HW;                 // one history slot
    const long npix = (long)B * HW;
    const long half = npix * cpad;                   // rows of one CFG half in x_next
    for (long p = blockIdx.x * (long)NT + threadIdx.x; p < npix; p += (long)gridDim.x * NT) {
        const int b = (int)(p / HW);
        const int px = (int)(p - (long)b * HW);
        const T* pu = pred + p * ld;                                  // unconditional half (or the only one)
        const T* pt = pred + (p + npix) * ld;                         // text half
        T* xo = x_next + p * cpad;
        for (int c = 0; c < C; ++c) {
            const long i = ((long)b * C + c) * HW + px;               // NCHW index of the latent element
            float g = to_f32(pu[c]);
            if (cfg) g = form(g_u, g, g_t, to_f32(pt[c]));           // axpby(out[:B], out[B:], 1 - g, g)
            float eps, base = sample[i];
            if (r.mode == 0) {                                        // counter 0: ets = [g], cur_sample = sample
                eps = g;
                cur[i] = base;
            } else if (r.mode == 1) {                                 // counter 1: (g + ets[-1]) / 2 on cur_sample
                eps = form(r.coef[1], ets[(r.rslot[0] & 3) * N + i], r.coef[0], g);
                base = cur[i];
            } else {                                                  // linear multistep over ets[-1 .. -nterms]
                eps = form(r.coef[1], ets[(r.rslot[0] & 3) * N + i], r.coef[0], g);
                const int nterms = min(r.nterms, 4);
                for (int k = 2; k < nterms; ++k) eps = form(r.coef[k], ets[(r.rslot[k - 1] & 3) * N + i], 1.f, eps);
            }
            if (r.wslot >= 0) ets[(r.wslot & 3) * N + i] = g;    // (slots masked: a bad table cannot write outside ets)
            if (r.vpred) eps = form(r.v_x, base, r.v_v, eps);       // eps = sqrt(a) v + sqrt(1 - a) x
            const float prev = form(r.eps_scale, eps, r.x_scale, base);
            sample[i] = prev;
            const T o = from_f32<T>(prev);
            xo[c] = o;
            if (cfg) xo[half + c] = o;
        }
        for (int c = C; c < cpad; ++c) {                              // padding channels, as nchw2nhwc_kernel leaves them
            xo[c] = from_f32<T>(0.f);
            if (cfg) xo[half + c] = from_f32<T>(0.f);
        }
    }
    if (blockIdx.x == 0 && step + 1 < nsteps) {                       // the next U-Net call's timesteps
        const int nt = cfg ? 2 * B : B;
        for (int j = threadIdx.x; j < nt; j += NT) t_out[j] = table[step + 1].t;
    }
    // advance the counter once every workgroup has read it: the last one to finish does it (and re-arms the ticket)
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(reinterpret_cast<unsigned*>(state + 1), 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (last && threadIdx.x == 0) {
        atomicExch(state + 1, 0);
        atomicExch(state, step + 1);
    }
}

// DDIM (eta 0): the step is linear in (sample, model output), so one table row is the timestep and DDIMScheduler.coefficients.
// Counter, ticket, t_out and x_next are plms_step_kernel's.
template <typename T>
__global__ void ddim_step_kernel(const T* __restrict__ pred, int ld, float g_u, float g_t, int cfg,
                                 float* __restrict__ sample, const pdmk_ddim_row* __restrict__ table, int nsteps,
                                 int32_t* state, int64_t* __restrict__ t_out, T* __restrict__ x_next, int cpad, int B, int C,
                                 int HW) {
    const int step = state[0];
    if (step < 0 || step >= nsteps) return;          // every workgroup reads the same counter: all of them return
    const float c_x = table[step].c_x, c_m = table[step].c_m;
    const long npix = (long)B * HW;
    const long half = npix * cpad;                   // rows of one CFG half in x_next
    for (long p = blockIdx.x * (long)NT + threadIdx.x; p < npix; p += (long)gridDim.x * NT) {
        const int b = (int)(p / HW);
        const int px = (int)(p - (long)b * HW);
        const T* pu = pred + p * ld;                                  // unconditional half (or the only one)
        const T* pt = pred + (p + npix) * ld;                         // text half
        T* xo = x_next + p * cpad;
        for (int c = 0; c < C; ++c) {
            const long i = ((long)b * C + c) * HW + px;               // NCHW index of the latent element
            float g = to_f32(pu[c]);
            if (cfg) g = form(g_u, g, g_t, to_f32(pt[c]));           // axpby(out[:B], out[B:], 1 - g, g)
            const float prev = form(c_m, g, c_x, sample[i]);          // axpby(model_output, prev, c_m, c_x)
            sample[i] = prev;
            const T o = from_f32<T>(prev);
            xo[c] = o;
            if (cfg) xo[half + c] = o;
        }
        for (int c = C; c < cpad; ++c) {                              // padding channels, as nchw2nhwc_kernel leaves them
            xo[c] = from_f32<T>(0.f);
            if (cfg) xo[half + c] = from_f32<T>(0.f);
        }
    }
    if (blockIdx.x == 0 && step + 1 < nsteps) {                       // the next U-Net call's timesteps
        const int nt = cfg ? 2 * B : B;
        for (int j = threadIdx.x; j < nt; j += NT) t_out[j] = table[step + 1].t;
    }
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(reinterpret_cast<unsigned*>(state + 1), 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (last && threadIdx.x == 0) {
        atomicExch(state + 1, 0);
        atomicExch(state, step + 1);
    }
}

// ROUND: diffusers' numpy_to_pil, `(img * 255).round().astype("uint8")` (rintf: half to even, as np.round)
template <bool ROUND>
__global__ void image_to_u8_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, int B, int C, int HW) {
    const long npix = (long)B * HW;
    for (long p = blockIdx.x * (long)NT + threadIdx.x; p < npix; p += (long)gridDim.x * NT) {
        const int b = (int)(p / HW);
        const int px = (int)(p - (long)b * HW);
        for (int c = 0; c < C; ++c) {
            float v = src[((long)b * C + c) * HW + px] / 2.f;       // torch: x / 2 (exact), then + 0.5 in its own kernel
            v = v + 0.5f;
            v = fminf(fmaxf(v, 0.f), 1.f);                            // clamp(0, 1); NaN -> 0
            v = v * 255.f;                                            // numpy float32 * 255
            if (ROUND) v = rintf(v);
            dst[p * C + c] = (uint8_t)(int)v;                         // astype(np.uint8) truncates
        }
    }
}

}  // namespace

extern "C" int pdmk_plms_step(const void* pred, int ld, float g_u, float g_t, int cfg, float* sample, float* cur, float* ets,
                              const pdmk_plms_row* table, int nsteps, int32_t* state, int64_t* t_out, void* x_next, int cpad,
                              int B, int C, int HW, int dtype, pdmk_stream s) {
    if (!pred || !sample || !cur || !ets || !table || !state || !t_out || !x_next || nsteps <= 0 || B <= 0 || C <= 0 ||
        HW <= 0 || ld < C || cpad < C)
        return -1;
    const dim3 grid(grid_for((long)B * HW));
    if (dtype == PDMK_BF16)
        hipLaunchKernelGGL(plms_step_kernel<bf16>, grid, dim3(NT), 0, (hipStream_t)s, (const bf16*)pred, ld, g_u, g_t, cfg,
                           sample, cur, ets, table, nsteps, state, t_out, (bf16*)x_next, cpad, B, C, HW);
    else if (dtype == PDMK_F32)
        hipLaunchKernelGGL(plms_step_kernel<float>, grid, dim3(NT), 0, (hipStream_t)s, (const float*)pred, ld, g_u, g_t, cfg,
                           sample, cur, ets, table, nsteps, state, t_out, (float*)x_next, cpad, B, C, HW);
    else return -2;
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_ddim_step(const void* pred, int ld, float g_u, float g_t, int cfg, float* sample,
                              const pdmk_ddim_row* table, int nsteps, int32_t* state, int64_t* t_out, void* x_next, int cpad,
                              int B, int C, int HW, int dtype, pdmk_stream s) {
    if (!pred || !sample || !table || !state || !t_out || !x_next || nsteps <= 0 || B <= 0 || C <= 0 || HW <= 0 || ld < C ||
        cpad < C)
        return -1;
    const dim3 grid(grid_for((long)B * HW));
    if (dtype == PDMK_BF16)
        hipLaunchKernelGGL(ddim_step_kernel<bf16>, grid, dim3(NT), 0, (hipStream_t)s, (const bf16*)pred, ld, g_u, g_t, cfg,
                           sample, table, nsteps, state, t_out, (bf16*)x_next, cpad, B, C, HW);
    else if (dtype == PDMK_F32)
        hipLaunchKernelGGL(ddim_step_kernel<float>, grid, dim3(NT), 0, (hipStream_t)s, (const float*)pred, ld, g_u, g_t, cfg,
                           sample, table, nsteps, state, t_out, (float*)x_next, cpad, B, C, HW);
    else return -2;
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_image_to_u8_ex(const float* src, uint8_t* dst, int B, int C, int HW, int rounding, pdmk_stream s) {
    if (!src || !dst || B <= 0 || C <= 0 || HW <= 0 || (rounding != 0 && rounding != 1)) return -1;
    const dim3 grid(grid_for((long)B * HW, 4096));
    if (rounding)
        hipLaunchKernelGGL(image_to_u8_kernel<true>, grid, dim3(NT), 0, (hipStream_t)s, src, dst, B, C, HW);
    else
        hipLaunchKernelGGL(image_to_u8_kernel<false>, grid, dim3(NT), 0, (hipStream_t)s, src, dst, B, C, HW);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_image_to_u8(const float* src, uint8_t* dst, int B, int C, int HW, pdmk_stream s) {
    return pdmk_image_to_u8_ex(src, dst, B, C, HW, 0, s);
}
