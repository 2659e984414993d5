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
// pdmk_sld_plms_step / pdmk_sld_ddim_step are the same two launches with Safe Latent Diffusion's three-branch guidance
// (sld_chain below: plain fp32 operations, no fma) in place of the axpby; pdmk_sld_guidance is that chain alone, for the
// eager loop.  pdmk_calg_plms_step / pdmk_calg_ddim_step are the same two launches with concept algebra's score projection on
// five branches (calg_chain below); its two scalars come from the fp64 partial sums that pdmk_calg_dots leaves, summed again
// by every workgroup in one fixed order.  pdmk_calg_guidance is that chain alone.  pdmk_lms_step / pdmk_sld_lms_step /
// pdmk_calg_lms_step are the launches for LMSDiscreteScheduler.step (K-LMS): the derivative and the update are axpby forms, and
// the next U-Net input is divided by sqrt(sigma^2 + 1) in the same launch (scale_model_input).  All nine step entry points are
// instances of one kernel (step_kernel<T, Guide, Sched>).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
inline int grid_for(long nwork, int cap = 1024) { return (int)max(1L, min((long)cap, (nwork + NT - 1) / NT)); }

__device__ __forceinline__ float form(float a, float x, float b, float y) { return __builtin_fmaf(a, x, b * y); }

// ---- guidance: what turns the U-Net's prediction rows into the scheduler's model output for NCHW element i (pixel p, channel c)
// Two branches (or none): pdmk_axpby(out[:B], out[B:], 1 - g, g).
struct CfgGuide {
    float g_u, g_t;
    int cfg;
    __device__ int copies() const { return cfg ? 2 : 1; }
    __device__ void prepare() {}
    template <typename T>
    __device__ float operator()(const T* __restrict__ pred, int ld, long p, long npix, int c, long, int) const {
        float g = to_f32(pred[p * ld + c]);                           // unconditional half (or the only one)
        if (cfg) g = form(g_u, g, g_t, to_f32(pred[(p + npix) * ld + c]));
        return g;
    }
};

// Safe Latent Diffusion (include/pdmk.h pdmk_sld_params): separate fp32 operations, each rounded once - what a torch fp32
// elementwise chain computes.  Nothing here is an fma (this file is compiled without contraction).  m is updated in place.
__device__ __forceinline__ float sld_chain(float u, float t, float s, float& m, float g, const pdmk_sld_params& q, bool apply) {
    const float d = t - s;
    float scale = fabsf(d) * q.sld_guidance_scale;
    scale = scale > 1.f ? 1.f : scale;                                // torch.clamp(max=1): NaN stays NaN
    if (d >= q.threshold) scale = 0.f;
    float gs = (s - u) * scale;
    const float mm = q.momentum_scale * m;
    gs = gs + mm;
    const float a = q.mom_beta * m, b = q.one_minus_beta * gs;
    m = a + b;
    float ng = t - u;
    if (apply) ng = ng - gs;
    const float gn = g * ng;
    return u + gn;
}

// Three branches, thirds in the order uncond, text, safety.  The warm-up is decided from the step counter.
struct SldGuide {
    float g;
    pdmk_sld_params q;
    float* mom;
    __device__ int copies() const { return 3; }
    __device__ void prepare() {}
    template <typename T>
    __device__ float operator()(const T* __restrict__ pred, int ld, long p, long npix, int c, long i, int step) const {
        return sld_chain(to_f32(pred[p * ld + c]), to_f32(pred[(p + npix) * ld + c]), to_f32(pred[(p + 2 * npix) * ld + c]),
                         mom[i], g, q, step >= q.warmup_steps);
    }
};

// Concept algebra (include/pdmk.h "Concept algebra"): the partial pairs of pdmk_calg_dots -> the two fp32 scalars.  One thread
// adds the pairs in index order and the workgroup takes the result from LDS, so every workgroup of every launch that reads the
// same workspace holds the same bits.  A sum of squares that is not finite, or whose root is zero in fp32, gives (0, 0): the
// chain then leaves the projection out.  Every thread of the workgroup must call this.
struct CalgScalars {
    float nrm, dot;
};
__device__ __forceinline__ CalgScalars calg_scalars(const double* __restrict__ ws, int nparts, float* scalars) {
    __shared__ float sc[2];
    if (threadIdx.x == 0) {
        double sdd = 0.0, swd = 0.0;
        for (int k = 0; k < nparts; ++k) sdd += ws[2 * k], swd += ws[2 * k + 1];
        const double root = sqrt(sdd);
        float nrm = (float)root, dot = (float)(swd / root);
        if (!(sdd - sdd == 0.0) || !(nrm > 0.f)) nrm = 0.f, dot = 0.f;
        sc[0] = nrm, sc[1] = dot;
        if (scalars && blockIdx.x == 0) scalars[0] = nrm, scalars[1] = dot;
    }
    __syncthreads();
    return CalgScalars{sc[0], sc[1]};
}

// Separate fp32 operations, each rounded once (no fma: this file is compiled without contraction).
__device__ __forceinline__ float calg_chain(float u, float t, float p0, float p1, float g, CalgScalars q) {
    float pw = 0.f;
    if (q.nrm > 0.f) {
        const float d = p1 - p0;
        const float e = d / q.nrm;
        pw = q.dot * e;
    }
    const float t2 = t - pw;
    const float ng = t2 - u;
    const float gn = g * ng;
    return u + gn;
}

// Five branches, fifths in the order uncond, text, p0, p1, p2 (p2 enters through the dot product only).
struct CalgGuide {
    float g;
    const double* ws;
    int nparts;
    float* scalars;
    CalgScalars q;
    __device__ int copies() const { return 5; }
    __device__ void prepare() { q = calg_scalars(ws, nparts, scalars); }
    template <typename T>
    __device__ float operator()(const T* __restrict__ pred, int ld, long p, long npix, int c, long, int) const {
        return calg_chain(to_f32(pred[p * ld + c]), to_f32(pred[(p + npix) * ld + c]), to_f32(pred[(p + 2 * npix) * ld + c]),
                          to_f32(pred[(p + 3 * npix) * ld + c]), g, q);
    }
};

// ---- schedulers: model output g of element i -> the previous sample, state updated in place
struct PlmsSched {
    float* sample;
    float* cur;
    float* ets;
    const pdmk_plms_row* table;
    using time_type = int64_t;
    __device__ int64_t t(int step) const { return table[step].t; }
    __device__ float next_input(int, float prev) const { return prev; }
    __device__ float operator()(int step, float g, long i, long N) const {
        const pdmk_plms_row& r = table[step];
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
        if (r.wslot >= 0) ets[(r.wslot & 3) * N + i] = g;        // (slots masked: a bad table cannot write outside ets)
        if (r.vpred) eps = form(r.v_x, base, r.v_v, eps);           // eps = sqrt(a) v + sqrt(1 - a) x
        const float prev = form(r.eps_scale, eps, r.x_scale, base);
        sample[i] = prev;
        return prev;
    }
};

// DDIM (eta 0): the step is linear in (sample, model output), so one table row is the timestep and DDIMScheduler.coefficients.
struct DdimSched {
    float* sample;
    const pdmk_ddim_row* table;
    using time_type = int64_t;
    __device__ int64_t t(int step) const { return table[step].t; }
    __device__ float next_input(int, float prev) const { return prev; }
    __device__ float operator()(int step, float g, long i, long) const {
        const float prev = form(table[step].c_m, g, table[step].c_x, sample[i]);      // axpby(model_output, prev, c_m, c_x)
        sample[i] = prev;
        return prev;
    }
};

// K-LMS (LMSDiscreteScheduler.step): the derivative d of this step goes into the 4-slot history, the update is the chain
// prev = sample + sum_j coef[j] d_{i-j}, newest first, each term one axpby.  An element's history is read and written by the
// thread that owns the element only.  The next U-Net input is scale_model_input of the NEXT step: prev / sqrt(sigma^2 + 1),
// one fp32 division.
struct LmsSched {
    float* sample;
    float* hist;
    const pdmk_lms_row* table;
    using time_type = float;
    __device__ float t(int step) const { return table[step].t; }
    __device__ float next_input(int step, float prev) const { return prev / table[step].in_div; }
    __device__ float operator()(int step, float g, long i, long N) const {
        const pdmk_lms_row& r = table[step];
        const float base = sample[i];
        const float d = r.dmode ? form(r.d_x, base, r.d_m, g) : g;     // v_prediction: sigma / (sigma^2 + 1) x + v / sqrt(sigma^2 + 1)
        hist[(r.wslot & 3) * N + i] = d;                                // (slots masked: a bad table cannot leave hist)
        float prev = form(r.coef[0], d, 1.f, base);
        const int nterms = min(r.nterms, 4);
        for (int j = 1; j < nterms; ++j) prev = form(r.coef[j], hist[(r.rslot[j - 1] & 3) * N + i], 1.f, prev);
        sample[i] = prev;
        return prev;
    }
};

// One launch between two U-Net calls: guidance, scheduler step, the next call's input (one copy per branch) and timesteps,
// and the step counter.  pdmk_plms_step, pdmk_ddim_step, pdmk_lms_step and their SLD and concept-algebra forms are its nine
// instances per dtype.  The scheduler types the timesteps (time_type) and maps the new sample to the next input (next_input).
template <typename T, typename Guide, typename Sched>
__global__ void step_kernel(const T* __restrict__ pred, int ld, Guide guide, Sched sched, int nsteps, int32_t* state,
                            typename Sched::time_type* __restrict__ t_out, T* __restrict__ x_next, int cpad, int B, int C,
                            int HW) {
    const int step = state[0];
    if (step < 0 || step >= nsteps) return;          // every workgroup reads the same counter: all of them return
    const long N = (long)B * C * HW;                 // one history slot
    const long npix = (long)B * HW;
    const long part = npix * cpad;                   // elements of one branch's rows in x_next
    const int copies = guide.copies();
    guide.prepare();                                 // (nothing for the guides without launch-wide scalars)
    for (long p = blockIdx.x * (long)NT + threadIdx.x; p < npix; p += (long)gridDim.x * NT) {
        const int b = (int)(p / HW);
        const int px = (int)(p - (long)b * HW);
        T* xo = x_next + p * cpad;
        for (int c = 0; c < C; ++c) {
            const long i = ((long)b * C + c) * HW + px;               // NCHW index of the latent element
            const float prev = sched(step, guide(pred, ld, p, npix, c, i, step), i, N);
            const T o = from_f32<T>(sched.next_input(step, prev));    // (the identity but for K-LMS's input scaling)
            for (int k = 0; k < copies; ++k) xo[k * part + c] = o;
        }
        for (int c = C; c < cpad; ++c)                                // padding channels, as nchw2nhwc_kernel leaves them
            for (int k = 0; k < copies; ++k) xo[k * part + c] = from_f32<T>(0.f);
    }
    if (blockIdx.x == 0 && step + 1 < nsteps) {                       // the next U-Net call's timesteps
        const int nt = copies * B;
        for (int j = threadIdx.x; j < nt; j += NT) t_out[j] = sched.t(step + 1);
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

template <typename Guide, typename Sched>
int launch_step(const void* pred, int ld, const Guide& guide, const Sched& sched, int nsteps, int32_t* state,
                typename Sched::time_type* t_out, void* x_next, int cpad, int B, int C, int HW, int dtype, pdmk_stream s) {
    const dim3 grid(grid_for((long)B * HW));
    if (dtype == PDMK_BF16)
        hipLaunchKernelGGL((step_kernel<bf16, Guide, Sched>), grid, dim3(NT), 0, (hipStream_t)s, (const bf16*)pred, ld, guide,
                           sched, nsteps, state, t_out, (bf16*)x_next, cpad, B, C, HW);
    else if (dtype == PDMK_F32)
        hipLaunchKernelGGL((step_kernel<float, Guide, Sched>), grid, dim3(NT), 0, (hipStream_t)s, (const float*)pred, ld, guide,
                           sched, nsteps, state, t_out, (float*)x_next, cpad, B, C, HW);
    else return -2;
    PDMK_CHECK_LAUNCH();
    return 0;
}

// The eager loop's SLD guidance on fp32 NCHW thirds: 16-byte loads and stores when n and the pointers allow.
template <int V>
__global__ void sld_guidance_kernel(const float* __restrict__ pred, float* __restrict__ out, float* __restrict__ mom, long n,
                                    float g, pdmk_sld_params q, int apply) {
    const long nv = n / V;
    for (long j = blockIdx.x * (long)NT + threadIdx.x; j < nv; j += (long)gridDim.x * NT) {
        float u[V], t[V], s[V], m[V], o[V];
        if (V == 4) {
            *reinterpret_cast<float4*>(u) = reinterpret_cast<const float4*>(pred)[j];
            *reinterpret_cast<float4*>(t) = reinterpret_cast<const float4*>(pred + n)[j];
            *reinterpret_cast<float4*>(s) = reinterpret_cast<const float4*>(pred + 2 * n)[j];
            *reinterpret_cast<float4*>(m) = reinterpret_cast<const float4*>(mom)[j];
        } else {
            u[0] = pred[j], t[0] = pred[n + j], s[0] = pred[2 * n + j], m[0] = mom[j];
        }
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = sld_chain(u[e], t[e], s[e], m[e], g, q, apply != 0);
        if (V == 4) {
            reinterpret_cast<float4*>(out)[j] = *reinterpret_cast<const float4*>(o);
            reinterpret_cast<float4*>(mom)[j] = *reinterpret_cast<const float4*>(m);
        } else {
            out[j] = o[0], mom[j] = m[0];
        }
    }
}

// pdmk_calg_dots: workgroup g's share of sum d d and sum w d, d = p1 - p0 and w = t - p2 in fp32, the sums in fp64.  Elements
// are taken in the latent's NCHW order i (thread j of workgroup g: i = g NT + j, then steps of gridDim NT), a thread's sum runs
// over its elements ascending, and the workgroup's 256 sums are added pairwise in LDS - one fixed order, no atomics.
constexpr int CALG_PARTS = 256;
inline int calg_parts(long n) { return grid_for(n, CALG_PARTS); }

template <typename T>
__global__ void __launch_bounds__(NT) calg_dots_kernel(const T* __restrict__ pred, int ld, int C, int HW, long n, long npix,
                                                       double* __restrict__ ws) {
    __shared__ double sdd[NT], swd[NT];
    double add = 0.0, awd = 0.0;
    const long chw = (long)C * HW;
    for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const long b = i / chw, r = i - b * chw;
        const int c = (int)(r / HW);
        const long p = b * HW + (r - (long)c * HW);
        const T* at = pred + p * ld + c;
        const long fifth = npix * ld;
        const float t = to_f32(at[fifth]), p0 = to_f32(at[2 * fifth]), p1 = to_f32(at[3 * fifth]), p2 = to_f32(at[4 * fifth]);
        const float d = p1 - p0, w = t - p2;
        add += (double)d * (double)d;
        awd += (double)w * (double)d;
    }
    sdd[threadIdx.x] = add, swd[threadIdx.x] = awd;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sdd[threadIdx.x] += sdd[threadIdx.x + h], swd[threadIdx.x] += swd[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) ws[2 * blockIdx.x] = sdd[0], ws[2 * blockIdx.x + 1] = swd[0];
}

// The eager loop's concept-algebra guidance on fp32 NCHW fifths: 16-byte loads and stores when n and the pointers allow.
template <int V>
__global__ void calg_guidance_kernel(const float* __restrict__ pred, float* __restrict__ out, long n, float g,
                                     const double* __restrict__ ws, int nparts, float* scalars) {
    const CalgScalars q = calg_scalars(ws, nparts, scalars);
    const long nv = n / V;
    for (long j = blockIdx.x * (long)NT + threadIdx.x; j < nv; j += (long)gridDim.x * NT) {
        float u[V], t[V], p0[V], p1[V], o[V];
        if (V == 4) {
            *reinterpret_cast<float4*>(u) = reinterpret_cast<const float4*>(pred)[j];
            *reinterpret_cast<float4*>(t) = reinterpret_cast<const float4*>(pred + n)[j];
            *reinterpret_cast<float4*>(p0) = reinterpret_cast<const float4*>(pred + 2 * n)[j];
            *reinterpret_cast<float4*>(p1) = reinterpret_cast<const float4*>(pred + 3 * n)[j];
        } else {
            u[0] = pred[j], t[0] = pred[n + j], p0[0] = pred[2 * n + j], p1[0] = pred[3 * n + j];
        }
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = calg_chain(u[e], t[e], p0[e], p1[e], g, q);
        if (V == 4)
            reinterpret_cast<float4*>(out)[j] = *reinterpret_cast<const float4*>(o);
        else
            out[j] = o[0];
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
    return launch_step(pred, ld, CfgGuide{g_u, g_t, cfg}, PlmsSched{sample, cur, ets, table}, nsteps, state, t_out, x_next, cpad,
                       B, C, HW, dtype, s);
}

extern "C" int pdmk_ddim_step(const void* pred, int ld, float g_u, float g_t, int cfg, float* sample,
                              const pdmk_ddim_row* table, int nsteps, int32_t* state, int64_t* t_out, void* x_next, int cpad,
                              int B, int C, int HW, int dtype, pdmk_stream s) {
    if (!pred || !sample || !table || !state || !t_out || !x_next || nsteps <= 0 || B <= 0 || C <= 0 || HW <= 0 || ld < C ||
        cpad < C)
        return -1;
    return launch_step(pred, ld, CfgGuide{g_u, g_t, cfg}, DdimSched{sample, table}, nsteps, state, t_out, x_next, cpad, B, C, HW,
                       dtype, s);
}

extern "C" int pdmk_sld_guidance(const float* pred, float* out, float* mom, int B, int C, int HW, float guidance_scale,
                                 const pdmk_sld_params* params, int apply, pdmk_stream s) {
    if (!pred || !out || !mom || !params || B <= 0 || C <= 0 || HW <= 0) return -1;
    const long n = (long)B * C * HW;
    const bool wide = n % 4 == 0 && ((uintptr_t)pred | (uintptr_t)out | (uintptr_t)mom) % 16 == 0;
    if (wide)
        hipLaunchKernelGGL(sld_guidance_kernel<4>, dim3(grid_for(n / 4)), dim3(NT), 0, (hipStream_t)s, pred, out, mom, n,
                           guidance_scale, *params, apply);
    else
        hipLaunchKernelGGL(sld_guidance_kernel<1>, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)s, pred, out, mom, n,
                           guidance_scale, *params, apply);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_sld_plms_step(const void* pred, int ld, float guidance_scale, const pdmk_sld_params* params, float* mom,
                                  float* sample, float* cur, float* ets, const pdmk_plms_row* table, int nsteps, int32_t* state,
                                  int64_t* t_out, void* x_next, int cpad, int B, int C, int HW, int dtype, pdmk_stream s) {
    if (!pred || !params || !mom || !sample || !cur || !ets || !table || !state || !t_out || !x_next || nsteps <= 0 || B <= 0 ||
        C <= 0 || HW <= 0 || ld < C || cpad < C)
        return -1;
    return launch_step(pred, ld, SldGuide{guidance_scale, *params, mom}, PlmsSched{sample, cur, ets, table}, nsteps, state, t_out,
                       x_next, cpad, B, C, HW, dtype, s);
}

extern "C" int pdmk_sld_ddim_step(const void* pred, int ld, float guidance_scale, const pdmk_sld_params* params, float* mom,
                                  float* sample, const pdmk_ddim_row* table, int nsteps, int32_t* state, int64_t* t_out,
                                  void* x_next, int cpad, int B, int C, int HW, int dtype, pdmk_stream s) {
    if (!pred || !params || !mom || !sample || !table || !state || !t_out || !x_next || nsteps <= 0 || B <= 0 || C <= 0 ||
        HW <= 0 || ld < C || cpad < C)
        return -1;
    return launch_step(pred, ld, SldGuide{guidance_scale, *params, mom}, DdimSched{sample, table}, nsteps, state, t_out, x_next,
                       cpad, B, C, HW, dtype, s);
}

extern "C" int64_t pdmk_calg_workspace_elems(int B, int C, int HW) {
    if (B <= 0 || C <= 0 || HW <= 0) return 0;
    return 2 * (int64_t)calg_parts((long)B * C * HW);
}

extern "C" int pdmk_calg_dots(const void* pred, int ld, int B, int C, int HW, int dtype, double* ws, int64_t ws_elems,
                              pdmk_stream s) {
    if (!pred || !ws || B <= 0 || C <= 0 || HW <= 0 || ld < C || ((uintptr_t)ws & 7) ||
        ws_elems < pdmk_calg_workspace_elems(B, C, HW))
        return -1;
    const long n = (long)B * C * HW, npix = (long)B * HW;
    const dim3 grid(calg_parts(n));
    if (dtype == PDMK_BF16)
        hipLaunchKernelGGL(calg_dots_kernel<bf16>, grid, dim3(NT), 0, (hipStream_t)s, (const bf16*)pred, ld, C, HW, n, npix, ws);
    else if (dtype == PDMK_F32)
        hipLaunchKernelGGL(calg_dots_kernel<float>, grid, dim3(NT), 0, (hipStream_t)s, (const float*)pred, ld, C, HW, n, npix, ws);
    else return -2;
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_calg_guidance(const float* pred, float* out, int B, int C, int HW, float guidance_scale, const double* ws,
                                  int64_t ws_elems, float* scalars, pdmk_stream s) {
    if (!pred || !out || !ws || B <= 0 || C <= 0 || HW <= 0 || ((uintptr_t)ws & 7) ||
        ws_elems < pdmk_calg_workspace_elems(B, C, HW))
        return -1;
    const long n = (long)B * C * HW;
    const int nparts = calg_parts(n);
    const bool wide = n % 4 == 0 && ((uintptr_t)pred | (uintptr_t)out) % 16 == 0;
    if (wide)
        hipLaunchKernelGGL(calg_guidance_kernel<4>, dim3(grid_for(n / 4)), dim3(NT), 0, (hipStream_t)s, pred, out, n,
                           guidance_scale, ws, nparts, scalars);
    else
        hipLaunchKernelGGL(calg_guidance_kernel<1>, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)s, pred, out, n,
                           guidance_scale, ws, nparts, scalars);
    PDMK_CHECK_LAUNCH();
    return 0;
}

extern "C" int pdmk_calg_plms_step(const void* pred, int ld, float guidance_scale, const double* ws, int64_t ws_elems,
                                   float* scalars, float* sample, float* cur, float* ets, const pdmk_plms_row* table, int nsteps,
                                   int32_t* state, int64_t* t_out, void* x_next, int cpad, int B, int C, int HW, int dtype,
                                   pdmk_stream s) {
    if (!pred || !ws || !sample || !cur || !ets || !table || !state || !t_out || !x_next || nsteps <= 0 || B <= 0 || C <= 0 ||
        HW <= 0 || ld < C || cpad < C || ((uintptr_t)ws & 7) || ws_elems < pdmk_calg_workspace_elems(B, C, HW))
        return -1;
    return launch_step(pred, ld, CalgGuide{guidance_scale, ws, calg_parts((long)B * C * HW), scalars, {0.f, 0.f}},
                       PlmsSched{sample, cur, ets, table}, nsteps, state, t_out, x_next, cpad, B, C, HW, dtype, s);
}

extern "C" int pdmk_calg_ddim_step(const void* pred, int ld, float guidance_scale, const double* ws, int64_t ws_elems,
                                   float* scalars, float* sample, const pdmk_ddim_row* table, int nsteps, int32_t* state,
                                   int64_t* t_out, void* x_next, int cpad, int B, int C, int HW, int dtype, pdmk_stream s) {
    if (!pred || !ws || !sample || !table || !state || !t_out || !x_next || nsteps <= 0 || B <= 0 || C <= 0 || HW <= 0 ||
        ld < C || cpad < C || ((uintptr_t)ws & 7) || ws_elems < pdmk_calg_workspace_elems(B, C, HW))
        return -1;
    return launch_step(pred, ld, CalgGuide{guidance_scale, ws, calg_parts((long)B * C * HW), scalars, {0.f, 0.f}},
                       DdimSched{sample, table}, nsteps, state, t_out, x_next, cpad, B, C, HW, dtype, s);
}

extern "C" int pdmk_lms_step(const void* pred, int ld, float g_u, float g_t, int cfg, float* sample, float* hist,
                             const pdmk_lms_row* table, int nsteps, int32_t* state, float* t_out, void* x_next, int cpad, int B,
                             int C, int HW, int dtype, pdmk_stream s) {
    if (!pred || !sample || !hist || !table || !state || !t_out || !x_next || nsteps <= 0 || B <= 0 || C <= 0 || HW <= 0 ||
        ld < C || cpad < C)
        return -1;
    return launch_step(pred, ld, CfgGuide{g_u, g_t, cfg}, LmsSched{sample, hist, table}, nsteps, state, t_out, x_next, cpad, B,
                       C, HW, dtype, s);
}

extern "C" int pdmk_sld_lms_step(const void* pred, int ld, float guidance_scale, const pdmk_sld_params* params, float* mom,
                                 float* sample, float* hist, const pdmk_lms_row* table, int nsteps, int32_t* state, float* t_out,
                                 void* x_next, int cpad, int B, int C, int HW, int dtype, pdmk_stream s) {
    if (!pred || !params || !mom || !sample || !hist || !table || !state || !t_out || !x_next || nsteps <= 0 || B <= 0 ||
        C <= 0 || HW <= 0 || ld < C || cpad < C)
        return -1;
    return launch_step(pred, ld, SldGuide{guidance_scale, *params, mom}, LmsSched{sample, hist, table}, nsteps, state, t_out,
                       x_next, cpad, B, C, HW, dtype, s);
}

extern "C" int pdmk_calg_lms_step(const void* pred, int ld, float guidance_scale, const double* ws, int64_t ws_elems,
                                  float* scalars, float* sample, float* hist, const pdmk_lms_row* table, int nsteps,
                                  int32_t* state, float* t_out, void* x_next, int cpad, int B, int C, int HW, int dtype,
                                  pdmk_stream s) {
    if (!pred || !ws || !sample || !hist || !table || !state || !t_out || !x_next || nsteps <= 0 || B <= 0 || C <= 0 ||
        HW <= 0 || ld < C || cpad < C || ((uintptr_t)ws & 7) || ws_elems < pdmk_calg_workspace_elems(B, C, HW))
        return -1;
    return launch_step(pred, ld, CalgGuide{guidance_scale, ws, calg_parts((long)B * C * HW), scalars, {0.f, 0.f}},
                       LmsSched{sample, hist, table}, nsteps, state, t_out, x_next, cpad, B, C, HW, dtype, s);
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
