"""Host side of pdm.pipelines.pruning_pipelines.LMSDiscreteScheduler (no GPU): the schedule, the exact coefficient integrals
against the restatement of diffusers' scheduler in tests/lms_fixtures.py, the step orders and ring slots of lms_rows(), the
strict from_config, load_scheduler's "lms" kind and the --scheduler flag of the four evaluation scripts."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lms_fixtures as LF  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (1, 2, 3, 5, 20, 50, 100)


def _sched(n, **kw):
    from pdm.pipelines.pruning_pipelines import LMSDiscreteScheduler
    s = LMSDiscreteScheduler(**kw)
    s.set_timesteps(n)
    return s


def test_schedule_100_steps():
    s = _sched(100)
    assert s.timesteps.dtype.is_floating_point and s.timesteps.numpy().dtype == np.float32
    assert np.array_equal(s.timesteps[:3].numpy(), np.array([999, 988.9091, 978.8182], dtype=np.float32))
    assert len(s.timesteps) == 100 and len(s.sigmas) == 101 and s.sigmas.dtype == np.float32
    np.testing.assert_allclose(s.sigmas[:3], [14.614647, 13.752514, 12.95247], rtol=1e-6)
    np.testing.assert_allclose(s.sigmas[-3:], [0.09870332, 0.02916753, 0], rtol=1e-6)
    assert s.init_noise_sigma == float(s.sigmas[0]) == float(s.sigmas.max())
    ref = LF.RefLMS()
    ref.set_timesteps(100)
    assert np.array_equal(ref.sigmas.numpy(), s.sigmas) and np.array_equal(ref.timesteps.numpy(), s.timesteps.numpy())
    assert s.derivatives == []


def _max_rel(how):
    worst = 0.0
    for n in STEPS:
        s = _sched(n)
        ref = LF.RefLMS()
        ref.set_timesteps(n)
        for i in range(n):
            order = min(i + 1, 4)
            got = s.lms_coefficients(i, order)
            assert len(got) == order
            for j in range(order):
                want = ref.get_lms_coefficient(order, i, j, how)
                worst = max(worst, abs(got[j] - want) / abs(want))
    return worst


def test_coefficients_equal_gauss_legendre():
    """The closed-form integrals against 4-point Gauss-Legendre (exact for cubics) on the same float64 sigmas, every c_j of
    every step for n in STEPS.  Largest relative difference measured on the CPU this was written on: 2.5e-15."""
    worst = _max_rel("gauss")
    print(f"LMS coefficients, exact integral vs Gauss-Legendre: max rel diff {worst:.3e}")
    assert worst <= 1e-12


def test_coefficients_equal_scipy_quad():
    """Against diffusers' own call, scipy.integrate.quad(..., epsrel=1e-4) on the fp32 sigma tensor, every c_j of every step for
    n in STEPS.  Largest relative difference measured on the CPU this was written on: 6.9e-7 (the integrand's fp32 rounding)."""
    pytest.importorskip("scipy")
    worst = _max_rel("quad")
    print(f"LMS coefficients, exact integral vs scipy quad: max rel diff {worst:.3e}")
    assert worst <= 1e-5


@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_orders_and_ring_slots(prediction_type):
    from pdm import _pdmk as k
    assert ctypes.sizeof(k.LmsRow) % 16 == 0
    for n in (1, 2, 3, 5, 10):
        s = _sched(n, prediction_type=prediction_type)
        rows = s.lms_rows()
        assert [r.nterms for r in rows] == [min(i + 1, 4) for i in range(n)]
        assert [r.t for r in rows] == s.timesteps.tolist()
        where = {}                                            # step -> slot that holds its derivative
        for i, r in enumerate(rows):
            reads = [r.rslot[j] for j in range(r.nterms - 1)]
            assert r.wslot not in reads and 0 <= r.wslot < 4
            assert reads == [where[i - 1 - j] for j in range(r.nterms - 1)], "a read finds the derivative of step i - 1 - j"
            where = {st: sl for st, sl in where.items() if sl != r.wslot}
            where[i] = r.wslot
            assert list(r.coef[:r.nterms]) == [np.float32(c) for c in s.lms_coefficients(i, r.nterms)]
            sig = np.float32(s.sigmas[i + 1])
            assert r.in_div == np.sqrt(sig * sig + np.float32(1))
            assert r.dmode == int(prediction_type == "v_prediction")
        assert rows[-1].in_div == 1.0


def test_from_config_is_strict(tmp_path):
    from pdm.pipelines.pruning_pipelines import LMSDiscreteScheduler
    ok = {"_class_name": "LMSDiscreteScheduler", "_diffusers_version": "0.21.0", "beta_start": 0.00085, "beta_end": 0.012,
          "beta_schedule": "scaled_linear", "num_train_timesteps": 1000, "trained_betas": None, "use_karras_sigmas": False,
          "prediction_type": "v_prediction", "timestep_spacing": "linspace", "steps_offset": 0}
    s = LMSDiscreteScheduler.from_config(ok)
    assert s.config.prediction_type == "v_prediction" and s.config.num_train_timesteps == 1000
    p = tmp_path / "scheduler_config.json"
    p.write_text(json.dumps(ok))
    assert LMSDiscreteScheduler.from_config(str(p)).config.prediction_type == "v_prediction"
    for bad in ({"use_karras_sigmas": True}, {"timestep_spacing": "leading"}, {"beta_schedule": "linear"},
                {"some_new_key": 1}):
        with pytest.raises(ValueError, match="not implemented"):
            LMSDiscreteScheduler.from_config({**ok, **bad})
    with pytest.raises(ValueError, match="prediction_type"):
        LMSDiscreteScheduler(prediction_type="sample")


def test_load_scheduler_lms_takes_prediction_type_and_betas_only(tmp_path):
    from pdm.pipelines.pruning_pipelines import LMSDiscreteScheduler
    from pdm.utils import load_models as LM
    from pdm.utils.config import Cfg
    d = tmp_path / "snap" / "scheduler"
    d.mkdir(parents=True)
    (d / "scheduler_config.json").write_text(json.dumps({
        "_class_name": "PNDMScheduler", "beta_start": 0.001, "beta_end": 0.02, "beta_schedule": "scaled_linear",
        "num_train_timesteps": 500, "prediction_type": "v_prediction", "skip_prk_steps": True, "set_alpha_to_one": False,
        "steps_offset": 1, "timestep_spacing": "leading", "clip_sample": False, "trained_betas": None}))
    s = LM.load_scheduler(Cfg.wrap({"pretrained_model_name_or_path": str(tmp_path / "snap")}), "lms")
    assert type(s) is LMSDiscreteScheduler and s.config.prediction_type == "v_prediction"
    assert s.config.num_train_timesteps == 500 and len(s.sigmas_all) == 500
    want = LMSDiscreteScheduler(num_train_timesteps=500, beta_start=0.001, beta_end=0.02)
    assert np.array_equal(s.sigmas_all, want.sigmas_all)
    s = LM.load_scheduler(Cfg(), "lms")
    assert type(s) is LMSDiscreteScheduler and s.config.prediction_type == "v_prediction" and len(s.sigmas_all) == 1000


def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_lms_host", os.path.join(
        ROOT, "unlearn-ft_amd", "scripts", "baselines", "unified_concept_editing", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name,argv", [
    ("generate_images", ["--model_name", "original", "--prompts_path", "p.csv", "--save_path", "out"]),
    ("sld_generate_images", ["--prompts_path", "p.csv", "--save_path", "out"]),
    ("concept_algebra", ["--model_name", "original", "--prompts_path", "p.csv", "--save_path", "out"]),
    ("debiasing_vl", ["--model_name", "original", "--prompts_path", "p.csv", "--save_path", "out"])])
def test_scheduler_flag(name, argv):
    mod = _script(name)
    assert mod.parse_args(argv).scheduler == "pndm"
    assert mod.parse_args(argv + ["--scheduler", "lms"]).scheduler == "lms"
    with pytest.raises(SystemExit):
        mod.parse_args(argv + ["--scheduler", "ddim"])
    assert "--scheduler lms" in mod.__doc__ and "DESIGN.md 9m" in mod.__doc__
