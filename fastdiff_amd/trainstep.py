"""One training step of the denoiser as one graph replay (INTEGRATION.md "Training").

What FastDiffTask runs per step -- theta_timestep_loss's draws (util.py:312-318), the forward, nn.MSELoss, backward(), clip_grad_norm_
(base_task.py:231-233), the NaN-gradient scan (trainer.py:320-327) and torch.optim.AdamW.step() (FastDiff.py:121-125) -- with every
per-step quantity kept in device memory (lvc_op.train_draw / mse_loss / adamw_multi over the C ABI's fd_train_draw, fd_mse_*,
fd_adamw_multi): the step index that keys the Philox draws, the loss, the gradient norm, the clip coefficient, AdamW's step count and
bias corrections, and whether the update is skipped because a gradient is not finite.  A captured step therefore draws fresh `ts` and
`z` on every replay, and the host never waits for the device:

    ts = fastdiff_amd.TrainStep(model, diffusion_hyperparams)          # base.yaml:98-103 are the defaults
    for mels, wavs in loader:
        loss = ts.step(mels, wavs)                                       # a device tensor; nothing synchronises
        if it % 100 == 0: print(ts.state())                              # this does

With a corpus in device memory (fastdiff_amd/corpus.py) the batch is cut inside the step as well (lvc_op.train_collate, keyed by the same
device-side step index as the draws), step() takes no argument and no byte of the batch crosses the bus:

    ts = fastdiff_amd.TrainStep(model, diffusion_hyperparams, corpus=corpus, batch_size=20)
    for it in range(steps):
        loss = ts.step()                                                 # ts.picked: the (item, start frame) of every slot

With ema_decay the step also keeps an exponential moving average of the parameters (fastdiff_amd/ema.py: ParamEMA; the reference has
none), updated behind the optimizer inside the same replay and only when the optimizer applied the step:

    ts = fastdiff_amd.TrainStep(model, diffusion_hyperparams, ema_decay=0.999)      # ts.ema; model.use_weights(ts.ema) vocodes from it

The library's scratch buffers are per device and grow by free + allocate: a captured step has their addresses baked in, so a LARGER
training call on the same device after the capture (a second TrainStep on a bigger model, a bigger batch through the eager training
path) invalidates it -- one model per process and device, as for the training operators in general (lvc_op._handle).
Single process, float32, one optimizer step per batch (no DDP, AMP, gradient accumulation, clip_grad_value or dropout: INTEGRATION.md).
"""
import torch

from . import lvc_op


class TrainStep:
    def __init__(self, model, diffusion_hyperparams, lr=2e-4, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.0, clip_grad_norm=1.0, seed=0,
                 graph=True, *, ema_decay=None, ema_warmup=True, corpus=None, batch_size=None, rank=0, world_size=1):
        self.model = model
        self._init_optimizer(list(model.parameters()), lr, betas, eps, weight_decay, clip_grad_norm)
        self.T_train = int(diffusion_hyperparams["T"])
        self.alpha = diffusion_hyperparams["alpha"].detach().to(self.device, torch.float32).contiguous()
        self.seed = int(seed)
        self.use_graph = bool(graph)
        self._graph = None
        self._init_batch_source(corpus, batch_size, rank, world_size)
        self.mel = self.wav = self.x_t = self.z = self.steps = None      # the static buffers of the current batch shape
        # the average of the parameters (None: off, and no launch of the step is about it)
        self.ema = None
        if ema_decay is not None:
            from .ema import ParamEMA
            self.ema = ParamEMA(model, decay=ema_decay, warmup=ema_warmup)

    def _init_optimizer(self, params, lr, betas, eps, weight_decay, clip_grad_norm):
        """AdamW's state over `params` on their device: the hyper-parameters, the fd_train_state, zeroed moments in two flat buffers."""
        self.params = params
        if not self.params or not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in self.params):
            raise RuntimeError(f"fastdiff_amd.{type(self).__name__} needs its parameters as contiguous float32 tensors on a HIP device (no CPU fallback)")
        self.device = self.params[0].device
        self.hyper = dict(lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps), weight_decay=float(weight_decay),
                          max_norm=float(clip_grad_norm or 0.0))
        self._hyper_dev = lvc_op.new_state("fd_adamw_hyper", self.device, torch.float64)
        self._write_hyper()
        self._state = lvc_op.new_train_state(self.device)                               # fd_train_state
        sizes = [p.numel() for p in self.params]
        self._m, self._v = (torch.zeros(sum(sizes), device=self.device, dtype=torch.float32) for _ in range(2))
        self.exp_avg = [t.view(p.shape) for t, p in zip(self._m.split(sizes), self.params)]
        self.exp_avg_sq = [t.view(p.shape) for t, p in zip(self._v.split(sizes), self.params)]

    def _init_batch_source(self, corpus, batch_size, rank, world_size):
        """The batch source of step(): rank / world_size only shape the plan (corpus.plan), the step itself stays single-process."""
        name = type(self).__name__
        self._key = self.loss = None      # the batch shape the buffers are for; the last loss
        self.corpus, self.batch_size, self.rank, self.world_size, self.picked = corpus, None, int(rank), int(world_size), None
        if corpus is not None:
            if batch_size is None or int(batch_size) < 1:
                raise ValueError(f"{name}: a corpus needs batch_size")
            if corpus.device != self.device:
                raise RuntimeError(f"{name}: the corpus lies on {corpus.device}, the parameters on {self.device} (corpus.to(device) uploads it)")
            if not 0 <= self.rank < self.world_size:
                raise ValueError(f"{name}: rank={rank} of world_size={world_size}")
            self.batch_size = int(batch_size)
            self.picked = torch.zeros((self.batch_size, 2), dtype=torch.int64, device=self.device)      # (item, start frame) of the last batch

    # ---- hyper-parameters and state ------------------------------------------------------------------------------------------------
    def _write_hyper(self):
        self._hyper_dev.copy_(lvc_op.pack_state("fd_adamw_hyper", torch.float64, **self.hyper))      # (the keys are the struct's fields)

    def set_lr(self, lr):
        """The learning rate of the following steps: a copy of 8 bytes into device memory, between two replays."""
        self.hyper["lr"] = float(lr)
        lvc_op.state_field(self._hyper_dev, "fd_adamw_hyper", "lr").copy_(torch.tensor([float(lr)], dtype=torch.float64))

    def state(self):
        """{"iter", "applied", "skipped", "grad_norm", "loss"} of the device's fd_train_state.  Synchronises."""
        return lvc_op.read_train_state(self._state)

    def _group_template(self):
        opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=self.hyper["lr"], betas=(self.hyper["beta1"], self.hyper["beta2"]),
                                eps=self.hyper["eps"], weight_decay=self.hyper["weight_decay"])
        return opt.state_dict()["param_groups"][0]

    def state_dict(self):
        """The layout of torch.optim.AdamW(model.parameters()).state_dict(): the reference's checkpoints keep it as `optimizer_states`
        (trainer.py:424-437), and a torch AdamW loads it.  `step` is the number of applied steps.  Synchronises."""
        st = self.state()
        step = float(st["applied"])
        group = self._group_template()
        group["params"] = list(range(len(self.params)))
        sd = {"state": {i: {"step": torch.tensor(step), "exp_avg": m.detach().clone(), "exp_avg_sq": v.detach().clone()}
                        for i, (m, v) in enumerate(zip(self.exp_avg, self.exp_avg_sq))},
              "param_groups": [group],
              # what torch's layout has no place for (torch.optim.AdamW.load_state_dict ignores the keys)
              "train_step": {"iter": st["iter"], "skipped": st["skipped"], "clip_grad_norm": self.hyper["max_norm"], "seed": self.seed}}
        if self.ema is not None:
            sd["ema"] = self.ema.state_dict()
        return sd

    def load_state_dict(self, sd):
        """From state_dict()'s layout, i.e. also from a torch.optim.AdamW over the same parameters (one parameter group).  A parameter
        without an entry starts from zero moments; the step count is the largest one found (torch keeps one per parameter, this
        optimizer one for all).  With state_dict()'s own "train_step" entry the draw counter, the skipped count and clip_grad_norm
        come back as saved; a dictionary that went through a torch optimizer has lost it, and the draw counter then continues at the
        step count -- after a run with skipped steps that repeats the draws of that many iterations -- while clip_grad_norm and the
        seed stay the constructor's.  With ema_decay: an "ema" entry (ParamEMA.state_dict()) is restored; without one the average starts
        again from the parameters as they are now -- load the module's state_dict first."""
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError("TrainStep.load_state_dict: one parameter group over the module's parameters is expected")
        g = groups[0]
        if g.get("amsgrad", False) or g.get("maximize", False):
            raise NotImplementedError("TrainStep: amsgrad / maximize are not implemented")
        self.hyper.update(lr=float(g["lr"]), beta1=float(g["betas"][0]), beta2=float(g["betas"][1]), eps=float(g["eps"]),
                          weight_decay=float(g["weight_decay"]))
        self._write_hyper()
        step = 0
        for i, key in enumerate(g["params"]):
            st = sd["state"].get(key)
            if st is None:
                self.exp_avg[i].zero_()
                self.exp_avg_sq[i].zero_()
                continue
            self.exp_avg[i].copy_(st["exp_avg"])
            self.exp_avg_sq[i].copy_(st["exp_avg_sq"])
            step = max(step, int(float(st["step"])))
        extra = sd.get("train_step") or {}
        if "clip_grad_norm" in extra:
            self.hyper["max_norm"] = float(extra["clip_grad_norm"])
            self._write_hyper()
        self._state.copy_(lvc_op.pack_state("fd_train_state", iter=int(extra.get("iter", step)), applied=step, skipped=int(extra.get("skipped", 0))))
        if self.ema is not None:
            if sd.get("ema") is not None:
                self.ema.load_state_dict(sd["ema"])
            else:
                self.ema.reset(seen_applied=step)

    # ---- the step ----------------------------------------------------------------------------------------------------------------------
    def _collate(self):
        lvc_op.train_collate(self.corpus, self.batch_size, seed=self.seed, state=self._state, rank=self.rank, world_size=self.world_size,
                             out=(self.mel, self.wav, self.picked))

    def _run(self, state, collate=False):
        """The calls of one step on the current stream; state: the fd_train_state the optimizer advances; collate: the batch comes
        from the corpus (it only reads the state, like the draw)."""
        if collate:
            self._collate()
        lvc_op.train_draw(self.wav, self.alpha, self.T_train, seed=self.seed, state=self._state, out=(self.x_t, self.z, self.steps))
        eps = self.model((self.x_t, self.mel, self.steps))
        loss = lvc_op.mse_loss(eps, self.z, state)
        loss.backward()
        grads = [None if p.grad is None else p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in self.params]
        lvc_op.adamw_multi(list(zip(self.params, grads, self.exp_avg, self.exp_avg_sq)), self._hyper_dev, state)
        if self.ema is not None:
            self.ema.update(state)
        return loss.detach()

    def _warm_up(self, collate=False):
        """Three steps outside the capture (the library's scratch buffers grow on first use, which a capture cannot contain) that leave
        no trace: the draws only read the state, and the optimizer runs on a spare state with one more item whose only gradient element
        is NaN -- every launch of the step happens, the guard keeps it from writing a parameter or a moment.  The average's launches
        run on the spare state and a spare fd_ema_state: no step was applied there, so the shadow and its record stay as they are."""
        spare = lvc_op.new_train_state(self.device)
        spare_ema = lvc_op.new_ema_state(self.device) if self.ema is not None else None
        poison = tuple(torch.full((1,), v, device=self.device) for v in (0.0, float("nan"), 0.0, 0.0))
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(3):
                self.model.zero_grad(set_to_none=True)
                if collate:
                    self._collate()
                lvc_op.train_draw(self.wav, self.alpha, self.T_train, seed=self.seed, state=self._state, out=(self.x_t, self.z, self.steps))
                loss = lvc_op.mse_loss(self.model((self.x_t, self.mel, self.steps)), self.z, spare)
                loss.backward()
                grads = [None if p.grad is None else p.grad.contiguous() for p in self.params]
                lvc_op.adamw_multi(list(zip(self.params, grads, self.exp_avg, self.exp_avg_sq)) + [poison], self._hyper_dev, spare)
                if self.ema is not None:
                    self.ema.update(spare, spare_ema)
        torch.cuda.current_stream(self.device).wait_stream(side)
        self.model.zero_grad(set_to_none=True)

    def _batch_of(self, mels, wavs):
        """(collate, (mel shape, wav shape)): which batch this call of step() is on -- cut from the corpus, or the caller's."""
        name = type(self).__name__
        if mels is None and wavs is None:
            if self.corpus is None:
                raise RuntimeError(f"{name}.step() without a batch needs a {name} built with corpus= and batch_size=")
            B, F = self.batch_size, self.corpus.frames
            return True, ((B, 80, F), (B, 1, F * self.corpus.hop_size))
        if mels is None or wavs is None:
            raise TypeError(f"{name}.step: mels and wavs, or neither")
        return False, (tuple(mels.shape), tuple(wavs.shape))

    def _prepare(self, mel_shape, wav_shape):
        B, L = wav_shape[0], wav_shape[-1]
        if len(wav_shape) != 3 or wav_shape[1] != 1 or L % 4 != 0:
            raise ValueError("TrainStep.step: wavs [B, 1, L] with L a multiple of 4")
        self._graph = self.loss = None
        self.mel = torch.empty(tuple(mel_shape), device=self.device, dtype=torch.float32)
        self.wav, self.x_t, self.z = (torch.empty((B, 1, L), device=self.device, dtype=torch.float32) for _ in range(3))
        self.steps = torch.empty((B, 1), device=self.device, dtype=torch.float32)

    def step(self, mels=None, wavs=None):
        """One training step on the batch (mels [B, 80, T], wavs [B, 1, T * hop]): draws, forward, loss, backward, clip, AdamW.  Returns
        the loss as a device tensor (overwritten by the next step) and does not synchronise.  With graph=True the first step at a
        batch shape warms up and captures; every later one is a copy of the batch into static buffers and one replay.
        Without arguments the batch is cut from the constructor's corpus inside the step (`picked` then holds its items and start
        frames, corpus.plan(state()["iter"], batch_size, seed, rank, world_size) says the same beforehand): a replay and nothing else."""
        if not (self.model.training and torch.is_grad_enabled()):
            raise RuntimeError("TrainStep.step needs the module in train() mode and gradients enabled")
        collate, shapes = self._batch_of(mels, wavs)
        key = shapes + (collate,)
        if key != self._key:
            self._prepare(*shapes)
            self._key = key
        if not collate:
            self.mel.copy_(mels, non_blocking=True)
            self.wav.copy_(wavs, non_blocking=True)
        # the optimizer writes the parameters through raw pointers, which no tensor version counts: tell the module that its inference
        # handle holds older weights (FastDiff._ready then refreshes them on the device before its next inference call)
        self.model._weights_dirty = True
        if not self.use_graph:
            self.model.zero_grad(set_to_none=True)
            self.loss = self._run(self._state, collate)
            return self.loss
        if self._graph is None:
            self._warm_up(collate)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self.loss = self._run(self._state, collate)
            self._graph = graph
        self._graph.replay()
        return self.loss
