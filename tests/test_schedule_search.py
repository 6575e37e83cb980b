"""noise_scheduling(search="device"): the greedy schedule search (util.py:254-288) with its state in device memory (fd_sched_init /
_begin / _update) against the golden of the reference function and, bit for bit, against the host loop on the same module and x_T --
with the stand-in predictor of the fixture, with a seeded fastdiff_amd.NoisePredictor, and through every way the search can stop."""
import numpy as np
import pytest
import torch

import fastdiff_amd
import synth
from conftest import load_golden
from fastdiff_amd import sampler

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    import gpu_common
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_common.make_model()


@pytest.fixture(scope="module")
def golden():
    return load_golden("noise_scheduling"), torch.from_numpy(load_golden("schedule")["train_alpha"])


@pytest.fixture()
def fixed_x_T(monkeypatch, golden):
    g, _ = golden

    def use(B=1):
        x = torch.from_numpy(g["x_T"].copy())
        x = torch.cat([x * (1.0 - 0.25 * b) for b in range(B)])      # item b: the recorded x_T, scaled
        monkeypatch.setattr(sampler, "std_normal", lambda size: x.clone().view(*size).cuda())
        return (B, 1, x.shape[-1])
    return use


def both(model, size, dh, mel, ddim=False):
    host = fastdiff_amd.noise_scheduling(model, size, dh, condition=mel, ddim=ddim)
    dev = fastdiff_amd.noise_scheduling(model, size, dh, condition=mel, ddim=ddim, search="device")
    assert dev.is_cuda and dev.dtype == host.dtype == torch.float32
    assert torch.equal(dev, host), (dev.tolist(), host.tolist())
    return dev


def test_the_golden_schedule_and_the_host_loop(model, golden, fixed_x_T):
    g, alpha = golden
    size = fixed_x_T()
    dh = {"N": int(g["N"]), "betaN": float(g["betaN"]), "alphaN": float(g["alphaN"]), "rho": float(g["rho"]), "alpha": alpha}
    mel = torch.from_numpy(g["mel"]).cuda()
    with pytest.raises(AttributeError):                        # the stock module has no noise_pred, on either path
        fastdiff_amd.noise_scheduling(model, size, dh, condition=mel, search="device")
    model.noise_pred = synth.stub_noise_pred
    try:
        for ddim in (False, True):
            key = "betas_ddim" if ddim else "betas_ddpm"
            betas = both(model, size, dh, mel, ddim)
            assert betas.shape == g[key + "_f64"].shape
            d64 = np.abs(betas.double().cpu().numpy() - g[key + "_f64"]).max()
            print(key, betas.tolist(), "max |d beta| vs f64 reference %.2e" % d64)
            assert d64 < 1e-5 * g[key + "_f64"].max()
    finally:
        del model.noise_pred


def test_with_a_noise_predictor_on_a_batch(model, golden, fixed_x_T):
    """B = 2: the R = 1 form of the network (one condition, the mean of the items' ratios)."""
    g, alpha = golden
    size = fixed_x_T(2)
    torch.manual_seed(7)
    model.noise_pred = fastdiff_amd.NoisePredictor().cuda()
    mel = torch.from_numpy(g["mel"]).cuda().expand(2, -1, -1).contiguous()
    try:
        for ddim in (False, True):
            dh = {"N": 6, "betaN": 0.5, "alphaN": 0.2, "rho": 1e-3, "alpha": alpha}
            betas = both(model, size, dh, mel, ddim)
            print("NoisePredictor, ddim =", ddim, betas.tolist())
            assert 1 <= betas.numel() <= 6
    finally:
        del model.noise_pred


@pytest.mark.parametrize("change,n_found", [({"alphaN": 0.999}, 1),          # alpha > 1 behind the first update: betaN alone
                                            ({"rho": 0.4}, 1),               # the first predicted beta (at most half of betaN) is below rho
                                            ({"N": 1}, 1),
                                            ({"alphaN": 1e-3}, None)])       # below alpha[-1]: the step is clamped to T - 1
def test_every_way_to_stop(model, golden, fixed_x_T, change, n_found):
    g, alpha = golden
    size = fixed_x_T()
    dh = dict({"N": 4, "betaN": 0.5, "alphaN": 0.2, "rho": 1e-3, "alpha": alpha}, **change)
    assert dh["alphaN"] != 1e-3 or dh["alphaN"] < float(alpha[-1])
    model.noise_pred = synth.stub_noise_pred
    try:
        for ddim in (False, True):
            betas = both(model, size, dh, torch.from_numpy(g["mel"]).cuda(), ddim)
            print(change, "ddim =", ddim, betas.tolist())
            assert n_found is None or betas.numel() == n_found
            assert float(betas[-1]) == np.float32(dh["betaN"])
    finally:
        del model.noise_pred


def test_more_than_64_steps_are_refused(model, golden, fixed_x_T):
    g, alpha = golden
    size = fixed_x_T()
    dh = {"N": 65, "betaN": 0.5, "alphaN": 0.2, "rho": 1e-3, "alpha": alpha}
    with pytest.raises(ValueError, match="64"):
        fastdiff_amd.noise_scheduling(model, size, dh, condition=torch.from_numpy(g["mel"]).cuda(), search="device")
