"""The denoiser under autograd: what `FastDiffTask._training_step` (FastDiff.py:44-49) differentiates through
`theta_timestep_loss` (util.py:291-325).

The inference path (fd_forward / fd_sample) is one hand-written pipeline with no saved activations; training needs them, and needs
gradients with respect to 175 parameter tensors.  Here the network is a graph of torch.autograd.Function nodes over the C ABI's training
operators (fastdiff_amd/lvc_op.py), forward and backward on HIP kernels:
  * the location-variable convolution, twelve per forward -- the operator the reference states as unfold + einsum over a
    [B, C, T, hop + 2, 3] view (modules.py:220-253) -- reading the predictor's kernel_conv output as frame-major operands
    (kernel_conv1d_frames -> location_variable_convolution_frames: no transposes between the two), and the gate behind it;
  * the 21 small 32-channel convolutions with their skip add, activations and bias (conv32), first_audio_conv / final_conv (conv7),
    the up-samplers (upsample), the skip tensors' fan-out (skip_fan);
  * the KernelPredictors: their front ends (input convolution + activation, residual stack, c + r) for all three blocks side by side
    in one node (predictor_fronts: a predictor never sees x, so the three latency-bound chains run as one), bias_conv likewise
    (kernel_conv1d_side_by_side), kernel_conv per block;
  * weight-norm of all 53 convolutions in one operator (weight_norm_all).
What stays on torch: the step embedding's five linear layers and swish, three broadcast adds, the loss (4 % of the step's kernel time).
The sub-modules of fastdiff_amd.FastDiff are real nn.Conv1d / nn.Linear holders with the reference's weight_g / weight_v
parametrisation, so the reference's optimizer, checkpointing and DDP wrapper see the module they expect.  FastDiff.forward takes this
path when autograd is recording and the module is in train() mode or an input requires a gradient; everything else stays on the
inference kernels.

`lvc` (tests only): a replacement for the HIP operator with the same signature, so that the structure around it can be pinned on
the reference's gradients on a machine without a GPU; the product never passes it.
"""
import threading

import torch
import torch.nn.functional as F

from . import lvc_op
from .sampler import calc_diffusion_step_embedding


def _swish(x):
    return x * torch.sigmoid(x)


class _Path:
    """Which operators one forward runs on, decided once (differentiable_forward) and handed to every helper.  hip: the product path --
    lvc_op's operators, called by name, each site behind its *_supported predicate and its switch, torch where those say no; else the
    CPU / test path: the caller's `lvc` and torch for the rest.  The switches are attributes of the module, read here and nowhere else;
    False puts a single piece of the product path back to its predecessor (A/B runs: tools/train_step_probe.py)."""

    def __init__(self, module, lvc):
        self.hip, self.lvc = lvc is None, lvc
        self.frames = getattr(module, "_train_frames", True)          # (False: the reference's kernel tensor between the two operators)
        self.fuse_act = getattr(module, "_train_fuse_act", True)      # (False: the predictor's LeakyReLUs as torch nodes)
        self.skip_fan = getattr(module, "_train_skip_fan", True)      # (False: autograd's own fan-out)
        self.stack = getattr(module, "_train_stack", True)            # (False: one node per pair)
        self.wn_all = getattr(module, "_train_wn_all", True)          # (False: one operator per convolution)
        self.fronts = getattr(module, "_train_fronts", True)          # (False: the predictors' front ends one by one)


class _ForwardWeights(threading.local):
    """conv module -> its effective weight for the forward being recorded (differentiable_forward: all of them from ONE operator).
    Per thread, and keyed on the module OBJECT (held alive by the key): forwards recorded concurrently by replicas in other threads
    neither see nor clear each other's entries, and a recycled id() can never hand out another module's weight."""

    def __init__(self):
        self.map = {}


_WN = _ForwardWeights()


def _stored_weight(m):
    """The stored weight of a conv holder (weight_v while weight-norm is attached): what the *_supported predicates read shapes from."""
    return m.weight_v if hasattr(m, "weight_v") else m.weight


def _conv_weight(m):
    """The effective weight of a conv module: g * v / ||v|| while weight-norm is attached (what its forward hook computes: on HIP
    tensors one operator for all convolutions of the module, lvc_op.weight_norm_all, else one launch of lvc_op.weight_norm each way per
    convolution), the plain weight after remove_weight_norm()."""
    w = _WN.map.get(m)
    if w is not None:
        return w
    if hasattr(m, "weight_g"):
        if m.weight_v.is_cuda:
            return lvc_op.weight_norm(m.weight_v, m.weight_g)
        return torch._weight_norm(m.weight_v, m.weight_g, 0)
    return m.weight


def _conv(m, x):
    """m(x) for a Conv1d holder: on HIP tensors the weight-norm runs on this repo's operator (the module's own hook would run torch's), and
    the two 7-tap convolutions at the ends of the network on theirs (fastdiff_amd.lvc_op.conv7)."""
    if x.is_cuda and m.kernel_size == (7,) and lvc_op.conv7_supported(x, _stored_weight(m)):
        return lvc_op.conv7(x, _conv_weight(m), m.bias)
    if x.is_cuda and hasattr(m, "weight_g"):
        return F.conv1d(x, _conv_weight(m), m.bias, stride=m.stride, padding=m.padding, dilation=m.dilation)
    return m(x)


def _on_conv32(path, x, m, centre_tap=False):
    """True if this 32 -> 32 convolution of x runs on lvc_op.conv32: a 3-tap one at its own dilation; centre_tap: a 1 x 1 one, which
    the caller pads with a zero tap either side (the predicate then reads the shape of that weight from a view: nothing is launched)."""
    if not path.hip:
        return False
    if centre_tap:
        return m.kernel_size == (1,) and m.in_channels == m.out_channels == 32 and \
            lvc_op.conv32_supported(x, _stored_weight(m).detach().expand(-1, -1, 3), 1)
    return lvc_op.conv32_supported(x, _stored_weight(m), m.dilation[0])


def _dblock(p, x, path, picked=False):
    """DiffusionDBlock.forward (modules.py:127-138); F.interpolate(size = L // factor) in its default nearest mode picks every
    factor-th sample.  The reference runs the 1 x 1 residual convolution at the full rate and then picks (modules.py:129-130); a
    1 x 1 convolution commutes with picking columns, so here it runs on the picked columns: 1 / factor of the work, the same values
    and the same gradients (only the picked columns ever receive one).  `layer(leaky_relu(x, 0.2))` is lvc_op.conv32 where it fits."""
    if not picked:                   # (picked: the caller's skip_fan has taken the columns already)
        size = x.shape[-1] // p.factor
        x = F.interpolate(x, size=size)
    rd = p.residual_dense
    if _on_conv32(path, x, rd, centre_tap=True):
        # the 1 x 1 residual convolution as the centre tap of a 3-tap one (zeros either side) on the same HIP operator, no activations
        residual = lvc_op.conv32(x, F.pad(_conv_weight(rd), (1, 1)), rd.bias, 1, pre_slope=1.0, post_slope=1.0)
    else:
        residual = _conv(rd, x)
    for layer in p.conv:
        if _on_conv32(path, x, layer):
            x = lvc_op.conv32(x, _conv_weight(layer), layer.bias, layer.dilation[0])
        else:
            x = _conv(layer, F.leaky_relu(x, 0.2))
    return x + residual


def _pair_chain(seq):
    """(convs, slope) if the Sequential is nothing but "convolution, LeakyReLU(slope)" pairs -- at least one, one slope throughout --
    between Dropout modules that do nothing (p = 0, or eval()); else None.  What the convolutions must be is the caller's to ask."""
    mods = [m for m in seq if not (isinstance(m, torch.nn.Dropout) and (m.p == 0 or not m.training))]
    convs, acts = mods[0::2], mods[1::2]
    if not (len(convs) == len(acts) >= 1 and
            all(isinstance(a, torch.nn.LeakyReLU) and a.negative_slope == acts[0].negative_slope for a in acts)):
        return None
    return convs, acts[0].negative_slope


def _front_spec(p):
    """(input conv, [stack convs], slope) if the predictor's front end is the model's: Sequential(Conv1d(80, 64, 5, padding 2), LeakyReLU)
    and a residual Sequential of Conv1d(64, 64, 3, padding 1) + LeakyReLU pairs between Dropout(p = 0) modules, one slope throughout."""
    ic = list(p.input_conv)
    if not (len(ic) == 2 and isinstance(ic[0], torch.nn.Conv1d) and isinstance(ic[1], torch.nn.LeakyReLU) and ic[0].kernel_size == (5,) and
            ic[0].padding == (2,) and ic[0].in_channels == 80 and ic[0].out_channels == 64):
        return None
    chain = _pair_chain(p.residual_conv)
    if chain is None or chain[1] != ic[1].negative_slope or not all(
            isinstance(m, torch.nn.Conv1d) and m.kernel_size == (3,) and m.padding == (1,) and m.dilation == (1,) and
            m.in_channels == 64 and m.out_channels == 64 for m in chain[0]):
        return None
    return ic[0], chain[0], chain[1]


def _kernel_predictor(p, front, cfg, path, hop):
    """KernelPredictor.forward (modules.py:320-343) -> (kernels, their gradient slots), bias, as_frames.  kernel_conv (64 -> 24576
    channels: the largest matrix product of the step) runs on the HIP operator where its shapes fit, else on the module's own convolution.
    as_frames (the product path): kernel_conv writes the LVC operator's frame-major operand order directly -- [B, layers, T, 6144]
    instead of the reference's [B, layers, 32, 64, 3, T] -- and reads the gradient that way (lvc_op: kernel_conv1d_frames).
    front = (c, the front end's output for it, bias_conv's): the latter two None unless computed for all predictors at once."""
    def fits(m, h):
        return path.hip and isinstance(m, torch.nn.Conv1d) and m.padding == (1,) and m.dilation == (1,) and \
            lvc_op.kernel_conv_supported(h, _stored_weight(m))

    def conv(m, h):      # a 64 -> M, k3 convolution of the predictor: the HIP operator where its shapes fit, else the module itself
        if fits(m, h):
            return lvc_op.kernel_conv1d(h, _conv_weight(m), m.bias)
        return _conv(m, h) if isinstance(m, torch.nn.Conv1d) else m(h)

    def run(seq, h):     # a Sequential of the predictor; "Conv1d, LeakyReLU" pairs run as ONE operator where the convolution fits
        mods, i = list(seq), 0
        while i < len(mods):
            m = mods[i]
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            if path.fuse_act and fits(m, h) and isinstance(nxt, torch.nn.LeakyReLU) and m.out_channels <= 512:
                h = lvc_op.kernel_conv1d(h, _conv_weight(m), m.bias, nxt.negative_slope)
                i += 2
            elif path.fuse_act and path.hip and isinstance(m, torch.nn.Conv1d) and isinstance(nxt, torch.nn.LeakyReLU) and \
                    m.padding == (2,) and m.dilation == (1,) and m.stride == (1,) and \
                    lvc_op.input_conv_supported(h, _stored_weight(m)):      # input_conv: Conv1d(80, 64, 5), LeakyReLU
                h = lvc_op.input_conv(h, _conv_weight(m), m.bias, nxt.negative_slope)
                i += 2
            else:
                h = conv(m, h)
                i += 1
        return h

    def stack(seq, h):   # a Sequential of nothing but "Conv1d(64, 64, 3), LeakyReLU(s)" pairs and Dropout(p = 0): ONE autograd node
        chain = _pair_chain(seq) if path.hip and path.fuse_act and path.stack else None
        if chain is None or not all(fits(m, h) and m.out_channels == 64 for m in chain[0]):
            return None
        return lvc_op.kernel_conv_stack(h, [_conv_weight(m) for m in chain[0]], [m.bias for m in chain[0]], chain[1])

    c, front_out, bias_out = front
    layers, cin, ks = cfg["lvc_layers_each_block"], cfg["inner_channels"], cfg["lvc_kernel_size"]
    cout = 2 * cin
    B, _, T = c.shape
    if front_out is not None:
        c = front_out
    else:
        c = run(p.input_conv, c)              # Conv1d 80 -> 64 k5, LeakyReLU(0.1)
        r = stack(p.residual_conv, c)         # Dropout(p = 0), Conv1d 64 -> 64 k3, LeakyReLU(0.1), Conv1d, LeakyReLU, three times
        if r is None:
            r = run(p.residual_conv, c)
        c = c + r
    kc = p.kernel_conv
    # the frames pair exists for the model's own shape only (fd_lvc_*_frames: Cin 32, Cout 64, ks 3, hop 8 / 64 / 256); any other
    # configuration the constructor accepts takes the reference's kernel tensor through the generic operator below
    if path.hip and path.frames and (cin, cout, ks) == (32, 64, 3) and hop in (8, 64, 256) and \
            lvc_op.kernel_conv_frames_supported(c, _stored_weight(kc)):
        kf = lvc_op.kernel_conv1d_frames(c, _conv_weight(kc), kc.bias)       # [B, layers, T, 6144]
        # bias_conv's output likewise: the operator reads a layer's [B, 64, T] slice where it lies and writes its gradient into one buffer
        bo = bias_out if bias_out is not None else conv(p.bias_conv, c)
        return lvc_op.split_layers(kf), lvc_op.split_layers(bo.contiguous().view(B, layers, cout, T)), True
    k = conv(kc, c)
    # the reference slices kernels[:, i] (modules.py:213-214), whose backward builds a zero tensor of all four layers per slice and
    # adds the four up; unbind hands autograd the same views and gets one stack back.  (One kernel_conv call per layer on that
    # layer's weight rows -- contiguous kernels, no stack -- measured slower: 18.3 vs 17.1 ms per step; the slices of the WEIGHT then
    # pay the same zero-fill-and-add in their backward.)
    k6 = k.contiguous().view(B, layers, cin, cout, ks, T)
    bo = bias_out if bias_out is not None else conv(p.bias_conv, c)
    # on the product path the slices are used where they lie and their gradients land in one buffer (lvc_op.split_layers)
    return lvc_op.split_layers(k6) if path.hip else (k6.unbind(1), None), bo.contiguous().view(B, layers, cout, T).unbind(1), False


def _torch_gate(x, y):
    C = x.shape[1]
    return x + torch.sigmoid(y[:, :C]) * torch.tanh(y[:, C:])


def _lvc_block(p, x, audio_down, front, cfg, path):
    """TimeAware_LVCBlock.forward (modules.py:189-218); the in-place `x += audio_down` of the reference written out of place.
    front: (the block's condition c + fc_t(emb), ...) as _kernel_predictor takes it."""
    hop = p.cond_hop_length
    (kernels, slots), bias, as_frames = _kernel_predictor(p.kernel_predictor, front, cfg, path, int(hop))
    if path.hip and x.is_cuda and lvc_op.upsample_supported(x, p.upsample):
        x = lvc_op.upsample(x, p.upsample.weight, p.upsample.bias, p.upsample.stride[0])      # leaky_relu + ConvTranspose1d in one HIP pass each way
    else:
        x = p.upsample(F.leaky_relu(x, 0.2))
    # audio_down: the skip tensor, or one alias of it per layer (lvc_op.skip_fan: their gradients are then added up in one pass)
    skip_of = (lambda i: audio_down[i]) if isinstance(audio_down, (list, tuple)) else (lambda i: audio_down)
    for i, conv in enumerate(p.convs):
        if _on_conv32(path, x, conv):
            # x += audio_down; leaky_relu; conv; leaky_relu (modules.py:209-212) in one HIP pass each way
            x, y = lvc_op.conv32(x, _conv_weight(conv), conv.bias, conv.dilation[0], skip=skip_of(i), post_slope=0.2)
        else:
            x = x + skip_of(i)
            y = F.leaky_relu(_conv(conv, F.leaky_relu(x, 0.2)), 0.2)
        if as_frames:
            y = lvc_op.location_variable_convolution_frames(y, kernels[i], bias[0][i], hop, grad_slot=slots[i], bias_slot=bias[1][i])
        elif path.hip:
            y = lvc_op.location_variable_convolution(y, kernels[i], bias[i], 1, hop, grad_slot=slots[i])
        else:
            y = path.lvc(y, kernels[i], bias[i], 1, hop)
        x = lvc_op.gated_residual(x, y) if path.hip else _torch_gate(x, y)      # x + sigmoid(y[:, :C]) * tanh(y[:, C:])  (modules.py:217)
    return x


def differentiable_forward(module, data, lvc=None):
    """eps = net((audio, c, diffusion_steps)) as FastDiff.forward (FastDiff_model.py:74-102), recorded by autograd."""
    path = _Path(module, lvc)
    _WN.map.clear()
    if path.hip and path.wn_all and data[0].is_cuda:
        n_mod = sum(1 for _ in module.modules())          # (the walk is cached while the module tree keeps its size: a convolution that
        cached = module.__dict__.get("_wn_candidates")    # is added or replaced later is picked up on the next step)
        if cached is None or cached[0] != n_mod or any(a is not b for a, b in zip(cached[2], module.modules())):
            mods_now = list(module.modules())
            cached = module.__dict__["_wn_candidates"] = (n_mod, [m for m in mods_now if isinstance(m, torch.nn.Conv1d)], mods_now)
        mods = [m for m in cached[1] if hasattr(m, "weight_g") and m.weight_v.is_cuda and
                m.weight_v.dtype == torch.float32 and m.weight_g.dtype == torch.float32 and m.weight_g.numel() == m.weight_v.shape[0]]
        if mods:
            for m, w in zip(mods, lvc_op.weight_norm_all([(m.weight_v, m.weight_g) for m in mods])):
                _WN.map[m] = w
    try:
        return _forward_body(module, data, path)
    finally:
        _WN.map.clear()


def _forward_body(module, data, path):
    audio, c, diffusion_steps = data
    cfg = module._cfg
    if c.dim() == 2:
        c = c.unsqueeze(0)
    emb = calc_diffusion_step_embedding(diffusion_steps.to(audio.dtype).view(audio.shape[0], 1), cfg["diffusion_step_embed_dim_in"])
    emb = _swish(module.fc_t2(_swish(module.fc_t1(emb))))
    x = _conv(module.first_audio_conv, audio)
    skips = []
    for down in module.downsample:
        if path.hip and path.skip_fan and len(module.lvc_blocks[0].convs) == 4 and lvc_op.skip_fan_supported(x, down.factor):
            picked, *aliases = lvc_op.skip_fan(x, down.factor)      # the DBlock's nearest pick + one alias of x per LVC layer that adds it
            skips.append(aliases)
            x = _dblock(down, picked, path, picked=True)
        else:
            skips.append(x)
            x = _dblock(down, x, path)
    blocks = module.lvc_blocks
    fronts = [None] * len(blocks)
    if path.hip and path.stack and path.fuse_act and c.is_cuda and c.dtype == torch.float32 and c.shape[1] == 80 and \
            1 <= c.shape[2] <= 128 and 2 <= len(blocks) <= 8 and path.fronts:
        # the KernelPredictors see only the mel and the step embedding, never x: their front ends -- input convolution + residual stack,
        # each a chain of latency-bound launches -- run side by side, one launch per chain step for all blocks (lvc_op.predictor_fronts)
        specs = [_front_spec(b.kernel_predictor) for b in blocks]
        if all(s is not None for s in specs) and len({(len(s[1]), s[2]) for s in specs}) == 1:
            conds = [c + b.fc_t(emb).unsqueeze(-1) for b in blocks]
            outs = lvc_op.predictor_fronts(conds, [(_conv_weight(s[0]), s[0].bias) for s in specs],
                                           [[(_conv_weight(m), m.bias) for m in s[1]] for s in specs], specs[0][2])
            fronts = list(zip(conds, outs, [None] * len(outs)))
            # ... and their bias_conv (64 -> 256, k3) likewise
            bcs = [b.kernel_predictor.bias_conv for b in blocks]
            if all(isinstance(m, torch.nn.Conv1d) and m.kernel_size == (3,) and m.padding == (1,) and m.dilation == (1,) and m.in_channels == 64 and
                   m.out_channels == bcs[0].out_channels and m.out_channels % 32 == 0 and m.out_channels <= 512 for m in bcs):
                fronts = list(zip(conds, outs, lvc_op.kernel_conv1d_side_by_side(outs, [_conv_weight(m) for m in bcs], [m.bias for m in bcs])))
    for n, audio_down in enumerate(reversed(skips)):
        front = fronts[n] or (c + blocks[n].fc_t(emb).unsqueeze(-1), None, None)      # (the block's condition, front end, bias_conv)
        x = _lvc_block(blocks[n], x, audio_down, front, cfg, path)
    return _conv(module.final_conv[0], x)
