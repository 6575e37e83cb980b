"""The scheduling network phi of BDDM on the MI355X (INTEGRATION.md "A schedule for your own weights").

The reference calls `net.noise_pred(x_t [B, L], (beta_next [R, 1], delta^2 [R, 1])) -> beta_hat [R, 1, 1]` from noise_scheduling and
phi_loss (util.py:284,356) but never defines it: the architecture here is THIS PROJECT'S OWN, not a port.  It keeps
BDDM's form  beta_hat = min(beta_next, delta^2) * sigma_phi(x):

    band energies   y[b,c,f] = band.bias[c] + sum_k band.weight[c,k] x[b, 32 f + k]      F = L / 32 - 1 frames of 64 samples, stride 32
                    feat[b,c] = log(1e-6 + mean_f y^2)                                    (the log after the mean: its gradient stays tame)
    head            in = (feat, ln beta_next, ln delta^2)   h = swish(fc1 in)   u = fc2 h
                    ratio = 1e-4 + (1 - 2e-4) sigmoid(u)    beta_hat = min(beta_next, delta^2) ratio

The clamp on ratio keeps delta^2 - beta_hat > 0 in phi_loss.  With one condition for a batch of several items (R = 1, B > 1: how
noise_scheduling calls it) the condition is broadcast and one value comes back, min(beta_next, delta^2) * mean_b ratio[b]; that form
exists only under no_grad.

    pred = fastdiff_amd.NoisePredictor().cuda()
    model.noise_pred = pred                      # the attribute the reference's functions look up

__call__ runs the HIP operators (lvc_op.band_pool / npred_head: fd_bandpool_*, fd_npred_head_*) forward and backward; there is no CPU
path.  reference_forward is the same network in plain torch operations in the dtype of its arguments: the float64 reference of the
tests, not a product path.
"""
import torch
from torch import nn

from . import lvc_op

N_BANDS, FRAME, HOP, HIDDEN = 32, 64, 32, 64
RATIO_MIN = 1e-4


class NoisePredictor(nn.Module):
    def __init__(self):
        super().__init__()
        self.band = nn.Linear(FRAME, N_BANDS)              # weight [32, 64], bias [32]: a bank of 32 learned analysis filters
        self.fc1 = nn.Linear(N_BANDS + 2, HIDDEN)           # [64, 34]
        self.fc2 = nn.Linear(HIDDEN, 1)                     # [1, 64]

    @staticmethod
    def _check(x, cond):
        beta_next, delta2 = cond
        if x.dim() != 2 or x.shape[1] < FRAME or x.shape[1] % HOP != 0:
            raise ValueError(f"NoisePredictor: x [B, L] with L a multiple of {HOP}, at least {FRAME}; got {tuple(x.shape)}")
        B, R = x.shape[0], beta_next.numel()
        if delta2.numel() != R or R not in (1, B):
            raise ValueError(f"NoisePredictor: cond = (beta_next [R, 1], delta2 [R, 1]) with R = B = {B} or R = 1")
        return B, R

    def forward(self, x, cond):
        """x [B, L], cond = (beta_next [R, 1], delta2 [R, 1]), R = B or 1 -> beta_hat [R, 1, 1].  HIP only."""
        if not x.is_cuda:
            raise RuntimeError("fastdiff_amd.NoisePredictor runs only on a HIP device (no CPU fallback); reference_forward is the torch form for tests")
        B, R = self._check(x, cond)
        if R != B and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("NoisePredictor: one condition for a batch of several items (R = 1) is allowed only under no_grad")
        beta_next, delta2 = (c.detach().reshape(-1) for c in cond)
        feat = lvc_op.band_pool(x.detach(), self.band.weight, self.band.bias)
        beta_hat, _ = lvc_op.npred_head(feat, beta_next, delta2, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias)
        return beta_hat.view(R, 1, 1)

    def features(self, x):
        """feat [B, 32] in plain torch operations, in x's dtype (part of reference_forward)."""
        w, b = self.band.weight.to(x.dtype), self.band.bias.to(x.dtype)
        frames = x.unfold(1, FRAME, HOP)                                      # [B, F, 64]
        y = torch.einsum("bfk,ck->bcf", frames, w) + b.view(1, -1, 1)
        return torch.log(1e-6 + (y * y).mean(-1))

    def reference_forward(self, x, cond):
        """The same network in plain torch operations, in the dtype of x (float64 in the tests).  Differentiable by torch's autograd."""
        B, R = self._check(x, cond)
        dt = x.dtype
        beta_next, delta2 = (c.to(dt).reshape(R, 1) for c in cond)
        feat = self.features(x)
        inp = torch.cat([feat, beta_next.log().expand(B, 1), delta2.log().expand(B, 1)], dim=1)
        a = inp @ self.fc1.weight.to(dt).t() + self.fc1.bias.to(dt)
        h = a * torch.sigmoid(a)
        u = h @ self.fc2.weight.to(dt).t() + self.fc2.bias.to(dt)
        ratio = RATIO_MIN + (1 - 2 * RATIO_MIN) * torch.sigmoid(u)            # [B, 1]
        scale = torch.minimum(beta_next, delta2)
        if R == B:
            return (scale * ratio).view(B, 1, 1)
        return (scale * (ratio.sum() / B)).view(1, 1, 1)
