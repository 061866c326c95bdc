"""Fused AdamW over the engines' flat trainable buffers (reference: ``optim.AdamW(model.parameters(), lr)`` at
scripts/train_cl.py:158 -- torch defaults betas (0.9, 0.999), eps 1e-8, weight_decay 0.01, applied to LoRA and head
weights *and biases*; frozen parameters have no gradient and are skipped)."""
import contextlib

import torch

from . import ops


class FusedAdamW(torch.optim.Optimizer):
    """Drop-in for ``torch.optim.AdamW``: same constructor, ``param_groups[0]['lr']`` honoured every step (so
    torch LR schedulers work).  Parameters that live in an engine ``FlatParams`` buffer are updated with one
    ``bsclip_adamw_step`` launch per buffer; any other trainable tensor gets its own launch of the same kernel.

    ``max_grad_norm`` / ``skip_nonfinite`` (``set_grad_clip``), both off by default: the global L2 norm of all flat
    gradients is formed on the device, the update runs on ``g * min(1, max_grad_norm / (norm + 1e-6))``
    (``torch.nn.utils.clip_grad_norm_``) and a step whose norm is not finite changes nothing -- parameters, moments and the step
    count stay (``GradScaler.step``).  No host read-back: eager and captured steps issue the same launches.

    ``ema_decay`` / ``ema_warmup`` (``set_ema``), off by default: an exponential moving average of the weights (timm's
    ``ModelEmaV2`` / ``V3``), one f32 buffer per flat buffer, moved inside the update launch (``bsclip_adamw_step_ema``) by the thread
    that stored the new weight; it follows the applied-step count, so a skipped step leaves it alone.  ``ema_weights()`` swaps it with
    the parameters in place for an evaluation or a checkpoint."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, skip_nonfinite=False,
                 ema_decay=None, ema_warmup=True):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._flat_state = {}
        self._flats = []
        self._dev_hyper = False
        self._shard = None        # (rank, world, group): optimizer-state sharding over the ranks (shard_state)
        self._clip_on = False
        self._max_norm = float("inf")
        self._clip_state = None       # int32 [12]: the device record of bsclip_grad_clip_finish
        self._clip_partials = None    # f64: every flat buffer's partial sums, one slice behind the other
        self._ema_decay = None        # None: no weight average
        self._ema_warmup = True
        self._ema_swapped = False     # inside ema_weights(): the flat buffers hold the average, st["ema"] the raw weights
        self.set_grad_clip(max_grad_norm, skip_nonfinite)
        self.set_ema(ema_decay, ema_warmup)

    _EMA_SHARDED = ("FusedAdamW: the weight average (EMA) cannot be kept with sharded optimizer state (shard_state): a slice owner "
                    "would average only its slice of every flat buffer")

    def set_ema(self, decay, warmup=True):
        """``decay``: keep ``ema = decay_t * ema + (1 - decay_t) * p`` after every applied step, a float strictly inside (0, 1) (None:
        off).  ``warmup``: ``decay_t = min(decay, (1 + t) / (10 + t))`` at applied step ``t`` (timm), else ``decay_t = decay``.  Call
        before the first step: the average starts as a copy of the weights that step finds."""
        if self._flat_state:
            raise RuntimeError("FusedAdamW.set_ema: call before the first step (the average starts from the initial weights and is "
                               "allocated with the moments)")
        if decay is not None:
            if isinstance(decay, bool) or not isinstance(decay, (int, float)):
                raise ValueError(f"FusedAdamW: ema_decay={decay!r} must be a float strictly inside (0, 1) (None: no average)")
            decay = float(decay)
            if not 0.0 < decay < 1.0:
                raise ValueError(f"FusedAdamW: ema_decay={decay!r} must be a float strictly inside (0, 1) (None: no average)")
            if self._shard is not None:
                raise RuntimeError(self._EMA_SHARDED)
        self._ema_decay = decay
        self._ema_warmup = bool(warmup)
        return self

    def ema_enabled(self):
        return self._ema_decay is not None

    def _ema_pairs(self):
        """(flat buffer, its average) of every valid flat buffer whose average exists (none before the first step)."""
        out = []
        for f in self._flats:
            if not f.valid():
                continue
            key = tuple(id(p) for p in f.params)
            st = self._flat_state.get(id(f)) or next((v for v in self._flat_state.values() if v.get("key") == key), None)
            if st is not None and "ema" in st and st["ema"].numel() == f.data.numel():
                out.append((f, st["ema"]))
        return out

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the parameters ARE the averaged weights: every flat buffer is swapped with its average in place
        (``bsclip_swap_f32``, one launch per buffer, no third buffer) and swapped back on exit, also when the block raises.  The
        engines read the flat buffers on every forward and a captured graph holds their addresses, which stay: nothing is rebuilt.
        Before the first step the average equals the weights and nothing is launched.  No step may run inside the block."""
        if self._ema_decay is None:
            raise RuntimeError("FusedAdamW.ema_weights: the weight average is off (ema_decay / set_ema)")
        if self._ema_swapped:
            raise RuntimeError("FusedAdamW.ema_weights: already inside an ema_weights() block")
        pairs = self._ema_pairs()
        if pairs and pairs[0][0].data.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamW.ema_weights: a stream is capturing (the swap belongs between replays, not into a graph)")
        for f, ema in pairs:
            ops.swap_f32(f.data, ema)
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._ema_swapped = False
            for f, ema in pairs:
                ops.swap_f32(f.data, ema)

    def ema_effective_decay(self):
        """``decay_t`` of the applied-step count reached so far, the decay the last applied step used (with skipping on: one
        read-back of the device's step word).  None when the average is off."""
        if self._ema_decay is None:
            return None
        st = next((s for s in self._flat_state.values() if "ema" in s), None)
        t = self._true_step(st) if st is not None else 0
        return min(self._ema_decay, (1.0 + t) / (10.0 + t)) if self._ema_warmup else self._ema_decay

    def set_grad_clip(self, max_grad_norm, skip_nonfinite=True):
        """``max_grad_norm``: clip the global gradient norm to it (None or +inf: no clipping).  ``skip_nonfinite``: leave parameters,
        moments and the step count untouched when the norm is Inf / NaN, and keep the statistics of ``grad_stats()``.  Clipping needs
        the skip: a non-finite norm cannot be clipped.  ``(None, False)`` is the plain optimizer.  The norm bound is a launch argument:
        set it before the step is captured."""
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:
                raise ValueError(f"FusedAdamW: max_grad_norm={max_grad_norm} must be positive (None: no clipping)")
            if not skip_nonfinite:
                raise ValueError("FusedAdamW: max_grad_norm needs skip_nonfinite=True (a non-finite gradient norm cannot be clipped)")
        if self._clip_on and not skip_nonfinite:
            self._refresh_steps_from_device()     # the host-side counts take over again
        self._clip_on = bool(skip_nonfinite)
        self._max_norm = float("inf") if max_grad_norm is None else max_grad_norm
        return self

    def grad_clip_enabled(self):
        return self._clip_on

    def _refresh_steps_from_device(self):
        """With the feature on the device step word counts APPLIED steps and the host's ``st["step"]`` attempted ones: bring the host
        count back to the device's (one read-back per flat buffer)."""
        if not self._clip_on:
            return
        for st in self._flat_state.values():
            if "hyper" in st:
                st["step"] = int(st["hyper"][1].item())

    def grad_stats(self, reset=False):
        """The gradient-norm record since the last reset, read back with one synchronisation: steps seen / skipped (non-finite norm) /
        clipped, mean and maximum of the finite norms, and the last step's norm and coefficient.  ``reset=True`` zeroes the counters
        and the sums behind the read (a stream-ordered fill)."""
        out = {"steps": 0, "skipped": 0, "clipped": 0, "norm_mean": 0.0, "norm_max": 0.0, "norm_last": 0.0, "coef_last": 1.0}
        if self._clip_state is None:
            return out
        w = self._clip_state.cpu().numpy()
        steps, skipped, clipped = (int(x) for x in w[4:7].view("uint32"))
        total, largest = (float(x) for x in w[8:12].view("float64"))
        applied = steps - skipped
        out.update(steps=steps, skipped=skipped, clipped=clipped, norm_mean=total / applied if applied else 0.0, norm_max=largest,
                   norm_last=float(w[2:3].view("float32")[0]), coef_last=float(w[1:2].view("float32")[0]))
        if reset:
            self._clip_state[4:].zero_()
        return out

    def shard_state(self, group=None):
        """Multi-rank full fine-tuning (every rank would otherwise hold the full 2 x 4 B per parameter of AdamW
        moments: 3.2 GB for I+D+T): each rank keeps the moments of ONE contiguous slice of every flat buffer and updates only
        that slice; after the update every slice is broadcast from its owner (``sync_updated_slices``, W small collectives per
        flat buffer -- they work on every backend and between graph replays).  Gradients are still all-reduced over the whole
        buffer (hip/dist.py), so the update itself is the unsharded one, element for element."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            self._shard = None
            return self
        if self._ema_decay is not None:
            raise RuntimeError(self._EMA_SHARDED)
        if self._flat_state:
            raise RuntimeError("FusedAdamW.shard_state: call before the first step (moments are already allocated unsharded)")
        self._shard = (dist.get_rank(group), dist.get_world_size(group), group)
        return self

    def _slice_of(self, f, rank=None):
        """[lo, hi) of flat buffer ``f`` owned by ``rank`` (default: this rank): equal 4-element-aligned slices, the last one short."""
        n = f.data.numel()
        if self._shard is None:
            return 0, n
        r, W, _ = self._shard
        r = r if rank is None else rank
        per = (-(-n // W) + 3) // 4 * 4
        return min(r * per, n), min((r + 1) * per, n)

    def sync_updated_slices(self):
        """Broadcast every rank's freshly updated parameter slice to the others.  Eager: called by ``step()`` outside a capture
        and by ``GraphedDistStep`` after its optimizer graph."""
        if self._shard is None:
            return
        import torch.distributed as dist
        _, W, group = self._shard
        works = []
        for f in self._flats:
            if not f.valid():
                continue
            for r in range(W):
                lo, hi = self._slice_of(f, r)
                if hi > lo:
                    works.append(dist.broadcast(f.data[lo:hi], src=dist.get_global_rank(group, r) if group is not None else r,
                                                group=group, async_op=True))
        for w in works:
            w.wait()

    def enable_device_hyper(self, on=True):
        """Read (lr, step) from device memory inside the kernel (``bsclip_adamw_step_dev``) instead of passing them as launch
        arguments: required when the step is captured into a hipGraph (arguments freeze at capture).  Each flat buffer owns a
        device pair ``[lr (f32), step (uint32)]``.  No in-flight node ever reads host memory: the step word is advanced on the
        device (eagerly it is set by a fill kernel carrying the value as a launch argument; under capture a
        ``bsclip_counter_add`` node advances it on every replay), and lr reaches the device through ``stage_hyper()`` -- a
        stream-ordered fill issued at call time, OUTSIDE the graph, before the replay that consumes it."""
        self._dev_hyper = bool(on)

    def _group_of(self, f):
        for g in self.param_groups:
            if any(p is f.params[0] for p in g["params"]):
                return g
        return self.param_groups[0]

    def _stage_lr(self, st, lr):
        """Enqueue ``lr`` into the lr word of one state's ``hyper`` pair unless it is what was staged last: a fill kernel whose value is
        a launch argument, stream-ordered behind the previous step, nothing for the host to overwrite while it is in flight.  Always
        issued OUTSIDE a graph (a captured fill would freeze the value): by an eager step, or before the replay that consumes it."""
        lr = float(lr)
        if st.get("lr_staged") != lr:
            st["hyper"].view(torch.float32)[0:1].fill_(lr)
            st["lr_staged"] = lr

    def _hyper_states(self):
        """(flat buffer, state) of every flat buffer that owns a device ``hyper`` pair."""
        states = ((f, self._flat_state.get(id(f))) for f in self._flats)
        return [(f, st) for f, st in states if st is not None and "hyper" in st]

    def stage_hyper(self):
        """Stage the current lr of every flat buffer's own param group into its device word (``_stage_lr``).  Called by ``GraphedStep``
        before each replay."""
        for f, st in self._hyper_states():
            self._stage_lr(st, self._group_of(f)["lr"])

    def advance_host_state(self):
        """Host half of one optimizer step, for a graph replay: the host's step counts follow the device words (which the
        replayed graph advances itself) and the current lr is staged."""
        for _, st in self._hyper_states():
            st["step"] += 1
        self.stage_hyper()

    def _true_step(self, st):
        """The step count of one flat buffer's state: the host's, or with skipping on the device word (applied steps only)."""
        if self._clip_on and "hyper" in st:
            return int(st["hyper"][1].item())
        return st["step"]

    def _state_for(self, f):
        """Adam moments of this rank's slice of one flat buffer (the whole buffer when unsharded).  Keyed by the PARAMETERS the buffer
        holds (they outlive an engine rebuild: a checkpoint loaded mid-run, a precision switch), not by the buffer object.  Unsharded,
        every parameter's part is also published in ``self.state[p]`` as views (``exp_avg``, ``exp_avg_sq``, ``step``) so
        ``state_dict()`` / ``load_state_dict()`` carry the moments like torch.optim.AdamW's do.  With the weight average on, ``ema``
        lives and travels with them: a copy of the parameters as the first step finds them, carried over a rebuild, restored from a
        loaded state."""
        key = tuple(id(p) for p in f.params)
        lo, hi = self._slice_of(f)
        st = self._flat_state.get(id(f))
        if st is not None and st["m"].numel() == hi - lo and st.get("key") == key:
            return st
        prev = next((v for v in self._flat_state.values() if v.get("key") == key and v.get("slice") == (lo, hi)), None)
        st = {"m": torch.zeros(hi - lo, dtype=f.data.dtype, device=f.data.device),
              "v": torch.zeros(hi - lo, dtype=f.data.dtype, device=f.data.device), "step": 0, "key": key, "slice": (lo, hi)}
        ema = self._ema_decay is not None
        if ema:
            st["ema"] = torch.empty(hi - lo, dtype=torch.float32, device=f.data.device)
            st["ema"].copy_(f.data[lo:hi])            # timm's deep copy at construction: the weights before the first update
        if prev is not None:                          # engine rebuilt (checkpoint loaded mid-run): the optimisation continues, it does not restart
            st["m"].copy_(prev["m"])
            st["v"].copy_(prev["v"])
            if ema and "ema" in prev:
                st["ema"].copy_(prev["ema"])
            st["step"] = self._true_step(prev)
        elif self._shard is None:                     # moments restored by load_state_dict() before the buffer existed
            for p, o in zip(f.params, f.offsets):
                ps = self.state.get(p)
                if ps and "exp_avg" in ps and ps["exp_avg"].numel() == p.numel():
                    st["m"][o:o + p.numel()].copy_(ps["exp_avg"].reshape(-1).to(st["m"].device))
                    st["v"][o:o + p.numel()].copy_(ps["exp_avg_sq"].reshape(-1).to(st["v"].device))
                    st["step"] = max(st["step"], int(ps.get("step", 0)))
                    if ema and "ema" in ps and ps["ema"].numel() == p.numel():
                        st["ema"][o:o + p.numel()].copy_(ps["ema"].reshape(-1).to(st["ema"].device))
        self._flat_state = {k: v for k, v in self._flat_state.items() if v.get("key") != key}
        self._flat_state[id(f)] = st
        if self._shard is None:
            for p, o in zip(f.params, f.offsets):
                self.state[p] = {"step": st["step"], "exp_avg": st["m"][o:o + p.numel()].view(p.shape),
                                 "exp_avg_sq": st["v"][o:o + p.numel()].view(p.shape)}
                if ema:
                    self.state[p]["ema"] = st["ema"][o:o + p.numel()].view(p.shape)
        return st

    def state_dict(self):
        if self._shard is not None:
            raise NotImplementedError("FusedAdamW: the moments are sharded over the ranks (shard_state); the reference checkpoints "
                                      "the model only (train_cl.py:219-220)")
        self._refresh_steps_from_device()             # skipped steps do not count (the device word is the true count)
        for f in self._flats:                         # the per-parameter step counts follow the flat buffer's
            st = self._flat_state.get(id(f))
            if st is not None:
                for p in f.params:
                    if p in self.state:
                        self.state[p]["step"] = st["step"]
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._flat_state = {}                         # next step(): moments are copied from self.state into the flat buffers

    def attach(self, model):
        """Tell the optimizer which engines' flat buffers exist (called by train_epoch after the first forward)."""
        from .dist import flat_buffers
        self._flats = flat_buffers(model)

    def needs_attach(self):
        """True until the engines' flat buffers are known, and again after an engine was rebuilt (checkpoint loaded mid-run)."""
        return not self._flats or not all(f.valid() for f in self._flats)

    def zero_grad(self, set_to_none: bool = True):
        handled = set()
        for f in self._flats:
            if f.valid():
                f.bind_grads()
                f.grad.zero_()
                handled.update(id(p) for p in f.params)
        for group in self.param_groups:
            for p in group["params"]:
                if id(p) in handled or p.grad is None:
                    continue
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def _norm_pass(self, flats, capturing):
        """The global gradient norm, eager and captured alike: one ``grad_sumsq_partial`` per flat buffer (over the WHOLE gradient, also
        when the update is sharded), then one ``grad_clip_finish``.  Returns the device record the updates are conditional on."""
        counts = [ops.grad_norm_partials(f.grad.numel()) for f in flats]
        total = sum(counts)
        dev = flats[0].grad.device
        if self._clip_state is None or self._clip_state.device != dev or self._clip_partials.numel() < total:
            if capturing:                             # a captured graph would hold a buffer of its private pool
                raise RuntimeError("FusedAdamW: run one eager step with gradient clipping / skipping on before capturing (its "
                                   "device buffers are allocated there)")
            if self._clip_state is None or self._clip_state.device != dev:
                self._clip_state = torch.zeros(ops.GRAD_CLIP_STATE_WORDS, dtype=torch.int32, device=dev)
            self._clip_partials = torch.empty(total, dtype=torch.float64, device=dev)
        off = 0
        for f, c in zip(flats, counts):
            f.bind_grads()
            ops.grad_sumsq_partial(f.grad, self._clip_partials[off:off + c])
            off += c
        ops.grad_clip_finish(self._clip_partials[:total], self._max_norm, self._clip_state)
        return self._clip_state

    def _step_flat(self, f, g, capturing, clip):
        """The update of this rank's slice of flat buffer ``f`` with param group ``g``'s hyperparameters: exactly one of ``adamw_step``
        (lr and step as launch arguments), ``adamw_step_dev`` (device hyper) and, with ``clip`` the norm pass's device record,
        ``counter_add_if`` + ``adamw_step_clip``; with the weight average on ``adamw_step_ema`` takes the place of all three (it reads
        lr and step from the device pair in every mode, and the record when there is one).  The step word of the ``hyper`` pair lives
        on the device so that no in-flight node ever reads host memory.  Device hyper: it is the host's count, set by a fill that carries the value as a launch argument, or
        under capture advanced by a ``counter_add`` node on every replay.  Clipping: it is filled once, when the pair is created, and
        from then on only advanced on the device, by ``counter_add_if``: it counts APPLIED steps, ``st["step"]`` attempted ones."""
        st = self._state_for(f)
        lo, hi = self._slice_of(f)
        ema = self._ema_decay is not None
        # device hyper: an empty slice launches nothing and gets no pair; clipping and the weight average: every buffer gets one (an
        # empty slice's stays as filled)
        if "hyper" not in st and (clip is not None or ema or (self._dev_hyper and hi > lo)):
            if capturing:
                raise RuntimeError("FusedAdamW: run one eager step with device-side (lr, step) before capturing (with the weight "
                                   "average on, its buffer is allocated there too)" if ema else
                                   "FusedAdamW: run one eager step with device-side (lr, step) before capturing")
            st["hyper"] = torch.zeros(2, dtype=torch.int32, device=f.data.device)   # [lr as f32 bits, step as uint32]
            if clip is not None:
                st["hyper"][1:2].fill_(st["step"])
        st["step"] += 1
        if hi <= lo:
            return
        fdata, fgrad = (f.data, f.grad) if self._shard is None else (f.data[lo:hi], f.grad[lo:hi])
        (beta1, beta2), eps, wd = g["betas"], g["eps"], g["weight_decay"]
        if clip is None and not self._dev_hyper and not ema:
            ops.adamw_step(fdata, fgrad, st["m"], st["v"], g["lr"], beta1, beta2, eps, wd, st["step"])
            return
        if clip is None:
            if capturing:
                ops.counter_add(st["hyper"][1:2], 1)              # a node of the graph: every replay advances the step word
            else:
                st["hyper"][1:2].fill_(st["step"])                 # value travels as a launch argument
        if not capturing:
            self._stage_lr(st, g["lr"])
        if clip is not None:
            ops.counter_add_if(st["hyper"][1:2], 1, clip[0:1])
        if ema:
            ops.adamw_step_ema(fdata, fgrad, st["m"], st["v"], st["ema"], st["hyper"], clip, beta1, beta2, eps, wd, self._ema_decay,
                               self._ema_warmup)
        elif clip is None:
            ops.adamw_step_dev(fdata, fgrad, st["m"], st["v"], st["hyper"], beta1, beta2, eps, wd)
        else:
            ops.adamw_step_clip(fdata, fgrad, st["m"], st["v"], st["hyper"], clip, beta1, beta2, eps, wd)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        in_opt = {id(p): g for g in self.param_groups for p in g["params"]}
        flats = [f for f in self._flats if f.valid() and all(id(p) in in_opt for p in f.params)]
        # asked once per step; a step on CPU tensors (the launch traces of tests/) cannot be under capture
        capturing = bool(flats) and flats[0].data.device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        handled = {id(p) for f in flats for p in f.params}
        loose = [(g, p) for g in self.param_groups for p in g["params"] if id(p) not in handled and p.grad is not None]
        if self._clip_on and loose:
            raise RuntimeError("FusedAdamW: gradient clipping / skipping needs every trainable tensor in an engine's flat "
                               "buffer (the norm is formed over the flat gradient buffers)")
        if self._ema_decay is not None:
            if self._shard is not None:
                raise RuntimeError(self._EMA_SHARDED)
            if loose:
                raise RuntimeError("FusedAdamW: the weight average (EMA) needs every trainable tensor in an engine's flat buffer (it "
                                   "is kept per flat buffer, inside the fused update)")
            if self._ema_swapped:
                raise RuntimeError("FusedAdamW: no step inside an ema_weights() block (the flat buffers hold the average there)")
        clip = self._norm_pass(flats, capturing) if self._clip_on and flats else None
        for f in flats:
            if clip is None:
                f.bind_grads()
            self._step_flat(f, in_opt[id(f.params[0])], capturing, clip)
        for g, p in loose:                            # a trainable tensor in no flat buffer: its own launch of the host-argument step
            if self._dev_hyper:
                raise RuntimeError("FusedAdamW: device-side (lr, step) needs every trainable tensor in an engine's flat buffer")
            if not (p.is_cuda and p.dtype == torch.float32 and p.data.is_contiguous() and p.grad.is_contiguous()):
                raise RuntimeError("FusedAdamW: parameters must be contiguous f32 GPU tensors (no CPU path)")
            st = self.state[p]
            if not st:
                st["m"], st["v"], st["step"] = torch.zeros_like(p.data), torch.zeros_like(p.data), 0
            st["step"] += 1
            ops.adamw_step(p.data.view(-1), p.grad.view(-1), st["m"].view(-1), st["v"].view(-1), g["lr"], g["betas"][0], g["betas"][1],
                           g["eps"], g["weight_decay"], st["step"])
        if self._shard is not None and not capturing:
            self.sync_updated_slices()
        return loss
