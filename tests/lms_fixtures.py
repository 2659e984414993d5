"""diffusers' LMSDiscreteScheduler restated operation by operation in torch / numpy on the CPU (no import of this package): what
tests/test_lms_scheduler_host.py and tests/test_lms_step_gpu.py hold pdm.pipelines.pruning_pipelines.LMSDiscreteScheduler
against.  diffusers is not installed where these tests are written, so this is a restatement of the published scheduler
(scaled_linear betas, linspace spacing, no Karras sigmas), not a pinned twin.

`dtype` is the precision of the latent arithmetic: torch.float32 is what diffusers runs (fp32 sigma scalars against fp32
tensors), torch.float64 the same operations on doubles - the yardstick of the accuracy test.  The sigmas hold fp32 values in
both."""
import numpy as np
import torch

_GL4_X = np.array([-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526])
_GL4_W = np.array([0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538])


class RefLMS:
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, prediction_type="epsilon",
                 dtype=torch.float32):
        self.T, self.prediction_type, self.dtype = num_train_timesteps, prediction_type, dtype
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)

    def set_timesteps(self, n):
        timesteps = np.linspace(0, self.T - 1, n, dtype=np.float32)[::-1].copy()
        sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()       # diffusers: np.array(...) of it
        sigmas = np.interp(timesteps, np.arange(0, len(sigmas)), sigmas)
        sigmas = np.concatenate([sigmas, [0.0]]).astype(np.float32)
        self.sigmas = torch.from_numpy(sigmas)                # fp32, as diffusers keeps them
        self.timesteps = torch.from_numpy(timesteps)
        self.init_noise_sigma = self.sigmas.max()
        self.derivatives = []

    def _sigma(self, i):
        return self.sigmas[i].to(self.dtype)

    def scale_model_input(self, sample, i):
        sigma = self._sigma(i)
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def lms_derivative(self, tau, order, t, current_order, sigmas):
        prod = 1.0
        for k in range(order):
            if current_order == k:
                continue
            prod *= (tau - sigmas[t - k]) / (sigmas[t - current_order] - sigmas[t - k])
        return prod

    def get_lms_coefficient(self, order, t, current_order, how="gauss"):
        """how "quad": diffusers' call, scipy.integrate.quad(..., epsrel=1e-4) of the integrand on the fp32 sigma tensor;
        "gauss": 4-point Gauss-Legendre on float64 copies of the sigmas - exact for the cubic (or lower) integrand."""
        if how == "quad":
            from scipy import integrate
            return integrate.quad(lambda tau: float(self.lms_derivative(tau, order, t, current_order, self.sigmas)),
                                  float(self.sigmas[t]), float(self.sigmas[t + 1]), epsrel=1e-4)[0]
        s = self.sigmas.numpy().astype(np.float64)
        a, b = s[t], s[t + 1]
        mid, half = 0.5 * (a + b), 0.5 * (b - a)
        return float(half * sum(w * self.lms_derivative(mid + half * x, order, t, current_order, s)
                                for x, w in zip(_GL4_X, _GL4_W)))

    def step(self, model_output, i, sample, order=4, how="gauss"):
        sigma = self._sigma(i)
        if self.prediction_type == "epsilon":
            pred_original_sample = sample - sigma * model_output
        else:
            pred_original_sample = model_output * (-sigma / (sigma ** 2 + 1) ** 0.5) + (sample / (sigma ** 2 + 1))
        derivative = (sample - pred_original_sample) / sigma
        self.derivatives.append(derivative)
        if len(self.derivatives) > order:
            self.derivatives.pop(0)
        order = min(i + 1, order)
        lms_coeffs = [self.get_lms_coefficient(order, i, curr_order, how) for curr_order in range(order)]
        return sample + sum(coeff * derivative for coeff, derivative in zip(lms_coeffs, reversed(self.derivatives)))


def seeded_run(prediction_type, dtype, steps=10, shape=(2, 4, 8, 12), seed=0):
    """(the restatement after set_timesteps, initial latents, per-step predictions, the sample after every step): predictions are
    seeded fp32 normals that do not depend on the sample, so any two implementations see the same inputs."""
    gen = torch.Generator().manual_seed(seed)
    ref = RefLMS(prediction_type=prediction_type, dtype=dtype)
    ref.set_timesteps(steps)
    lat = torch.randn(shape, generator=gen) * ref.init_noise_sigma
    preds = [torch.randn(shape, generator=gen) for _ in range(steps)]
    x, out = lat.to(dtype), []
    for i in range(steps):
        x = ref.step(preds[i].to(dtype), i, x)
        out.append(x)
    return ref, lat, preds, out
