"""Fused AdamW (csrc/kernels/fused_adamw.hip) with optional fused global-norm
clipping and three rounding modes, and the gradient norm / clip entry points
(csrc/kernels/grad_norm.hip). On a HIP device these run the in-tree kernels;
on the CPU, and for parameters that are not bf16, plain torch with the same
semantics (``adamw_ref.py`` has the stochastic bits)."""

from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional

import torch

from torchft_amd.ops import hip_ext
from torchft_amd.ops.adamw_ref import sr_bits, stochastic_round_bf16


def _local_view(t: torch.Tensor) -> torch.Tensor:
    """The local shard of a DTensor (FSDP2 sharded params/grads), else t.
    The update runs on the shard in place — mathematically identical for
    elementwise optimizers, and what lets the HSDP path use the fused
    kernel."""
    try:
        from torch.distributed.tensor import DTensor
    except ImportError:  # pragma: no cover
        return t
    return t.to_local() if isinstance(t, DTensor) else t


_GRAD_NORM_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _sumsq_torch(tensors: List[torch.Tensor]) -> torch.Tensor:
    """Plain-torch sum of squares (double accumulation) as fp32 [1]."""
    total = torch.zeros((), dtype=torch.float64, device=tensors[0].device)
    for t in tensors:
        total = total + t.detach().double().pow(2).sum()
    return total.float().reshape(1)


def _as_grads(tensors_or_params) -> List[torch.Tensor]:
    """Gradients to measure: a tensor that requires grad is a parameter and
    contributes its ``.grad`` (skipped if None); any other tensor is taken as
    a gradient itself. DTensors contribute their local shard."""
    if isinstance(tensors_or_params, torch.Tensor):
        tensors_or_params = [tensors_or_params]
    out = []
    for t in tensors_or_params:
        if t.requires_grad:
            t = t.grad
            if t is None:
                continue
        t = _local_view(t)
        if t.numel() > 0:
            out.append(t)
    return out


def _use_hip_norm(grads: List[torch.Tensor]) -> bool:
    if not grads[0].is_cuda:
        return False
    for g in grads:
        if g.dtype not in _GRAD_NORM_DTYPES:
            raise TypeError(f"grad norm kernel: unsupported dtype {g.dtype}")
    return True


def grad_norm(tensors_or_params, *, norm_reduce=None, max_blocks: int = 2048) -> torch.Tensor:
    """Global L2 norm of a list of gradients (or of the ``.grad`` of a list of
    parameters) as a 0-dim fp32 tensor on their device; no host sync.

    On a HIP device: csrc/kernels/grad_norm.hip, two launches and no atomics,
    so the value is bitwise reproducible for a given ``max_blocks`` (the cap
    on the reduction grid). ``norm_reduce``, if given, is called with the
    1-element fp32 sum of squares before the square root — sharded callers
    all-reduce (SUM) it there. On CPU: plain torch.

    The sum of squares is an fp32 number: finite gradients whose squares add
    up past 2**128 (``|g| >= 2**64`` in bf16 or fp32) give an ``inf`` norm.
    ``clip_grad_norm_`` then leaves the gradients untouched and
    ``FusedAdamW(max_grad_norm=...)`` skips the step and counts it, as for a
    non-finite gradient (docs/KERNELS.md, "Overflow rule").
    """
    grads = _as_grads(tensors_or_params)
    if not grads:
        raise ValueError("grad_norm: no gradients")
    if _use_hip_norm(grads):
        sumsq = hip_ext().grad_sumsq(grads, max_blocks)
    else:
        sumsq = _sumsq_torch(grads)
    if norm_reduce is not None:
        norm_reduce(sumsq)
    return sumsq.sqrt().reshape(())


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm: float, *, norm_reduce=None) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` for users of other optimizers:
    scales every ``.grad`` in place by ``min(1, max_norm / (norm + 1e-6))``
    and returns the pre-clip global norm as a 0-dim fp32 device tensor.
    Gradients are left untouched when the norm is non-finite, and nothing
    waits on the host. ``norm_reduce`` as in :func:`grad_norm`.
    """
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [_local_view(p.grad) for p in parameters if p.grad is not None]
    grads = [g for g in grads if g.numel() > 0]
    if not grads:
        raise ValueError("clip_grad_norm_: no gradients")
    max_norm = float(max_norm)
    if not max_norm > 0:
        raise ValueError(f"max_norm must be > 0, got {max_norm}")
    if _use_hip_norm(grads):
        sumsq = hip_ext().clip_grad_norm(grads, max_norm, 2048, norm_reduce)
        return sumsq.sqrt().reshape(())
    sumsq = _sumsq_torch(grads)
    if norm_reduce is not None:
        norm_reduce(sumsq)
    norm = sumsq.sqrt().reshape(())
    coef = (max_norm / (norm + 1e-6)).clamp(max=1.0)
    coef = torch.where(torch.isfinite(norm), coef, torch.ones_like(coef))
    for g in grads:
        g.mul_(coef)
    return norm


class _Rows(NamedTuple):
    """Parallel lists over the parameters of a step, those that have a
    gradient: local views, their state, and what the rounding mode brings.
    ``masters`` is empty unless the mode is master, ``stream_ids`` unless it is
    stochastic. ``states`` are the ``state[p]`` dicts the rest was read from."""

    params: List[torch.Tensor]
    grads: List[torch.Tensor]
    exp_avgs: List[torch.Tensor]
    exp_avg_sqs: List[torch.Tensor]
    steps: list
    masters: List[torch.Tensor]
    stream_ids: List[int]
    states: List[dict]

    def pick(self, idx: List[int]) -> "_Rows":
        """The rows ``idx``; a list that is empty stays empty."""
        return _Rows(*([col[i] for i in idx] if col else [] for col in self))


class FusedAdamW(torch.optim.Optimizer):
    """Single-kernel multi-tensor AdamW for bf16 params (fp32 moments).

    One launch per step updates every parameter (csrc/kernels/fused_adamw.hip);
    falls back to torch's foreach AdamW path on CPU. DTensor params (the
    FSDP2 sharded path) are updated on their local shards.

    ``max_grad_norm`` (opt-in; ``math.inf`` allowed) turns on the clip mode:
    the global L2 norm over all param groups is reduced on the device
    (csrc/kernels/grad_norm.hip), the clip coefficient is folded into the
    update's gradient read, and a non-finite norm skips the step on the
    device — ``p``, ``exp_avg``, ``exp_avg_sq`` and the bias-correction step
    stay untouched, with no host sync. In this mode ``state[p]["step"]`` is a
    0-dim int32 device tensor, ``last_grad_norm`` holds the pre-clip norm of
    the last step (non-finite if it was skipped) and ``skipped_steps`` counts
    the skips, both as device tensors. ``norm_reduce``, if given, is called
    with the 1-element fp32 sum of squares before the update; FSDP2/DTensor
    callers all-reduce (SUM) their shard's value there.

    ``rounding`` is how the fp32 result of the step reaches a bf16 parameter
    (docs/KERNELS.md, "Rounding modes"), in the plain and in the clip mode:

    ``"nearest"`` (default)  one round-to-nearest store, 22 B/element. An update
        below ``2^-9 |p|`` is dropped whole, step after step: fine while the
        learning rate is large, a stall late in a decaying schedule, and
        weight decay alone (``lr * wd`` of ``|p|``) never acts.
    ``"stochastic"``  the store rounds up or down at random with the expected
        value of the fp32 result, so small updates act on average. Same
        memory and traffic as ``"nearest"``; for pure-bf16 training that
        cannot afford four more bytes per parameter. The bits are
        Philox4x32-10 of (``sr_seed``, step count, the parameter's index in
        ``param_groups`` order, element index), so a run is reproducible and a
        checkpoint continues it bit for bit.
    ``"master"``  ``state[p]["master"]`` holds the parameter in fp32; the step
        runs on it and ``p`` is its bf16 rounding: what FSDP2 / torchtitan
        mixed precision gives, for 4 B/parameter more memory and 30 B/element
        of traffic. Where ``p`` no longer is the rounding of ``master``
        (DiLoCo's outer step, a heal, ``p.copy_()``), the step starts from
        ``p``, element by element, so nobody has to tell the optimizer.

    Parameters that are not bf16, and everything on the CPU, take the torch
    path with the same semantics.
    """

    ROUNDINGS = ("nearest", "stochastic", "master")

    def __init__(
        self,
        params,
        lr: float = 1e-3,
        betas=(0.9, 0.95),
        eps: float = 1e-8,
        weight_decay: float = 0.01,
        max_grad_norm: Optional[float] = None,
        norm_reduce: Optional[Callable[[torch.Tensor], None]] = None,
        rounding: str = "nearest",
        sr_seed: int = 0,
    ) -> None:
        if rounding not in self.ROUNDINGS:
            raise ValueError(f"rounding must be one of {self.ROUNDINGS}, got {rounding!r}")
        if not 0 <= int(sr_seed) < 2 ** 63:
            raise ValueError(f"sr_seed must be in [0, 2**63), got {sr_seed}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        if rounding == "stochastic":
            defaults["sr_seed"] = int(sr_seed)  # travels in state_dict()
        super().__init__(params, defaults)
        self.rounding = rounding
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0:
                raise ValueError(f"max_grad_norm must be > 0, got {max_grad_norm}")
        elif norm_reduce is not None:
            raise ValueError("norm_reduce needs max_grad_norm (math.inf to only report)")
        self.max_grad_norm = max_grad_norm
        self.norm_reduce = norm_reduce
        self.last_grad_norm: Optional[torch.Tensor] = None
        self.skipped_steps: Optional[torch.Tensor] = None
        if max_grad_norm is not None:
            dev = _local_view(self.param_groups[0]["params"][0]).device
            self._clip_buffers(dev)

    def _clip_buffers(self, dev: torch.device) -> None:
        skipped = self.skipped_steps
        self._sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
        self.skipped_steps = torch.zeros((), dtype=torch.int32, device=dev)
        if skipped is not None:  # params moved since construction
            self.skipped_steps.copy_(skipped)

    def load_state_dict(self, state_dict) -> None:  # noqa: D102
        # torch leaves a "step" entry as it was saved (an int or a tensor on
        # any device); make it what this optimizer's mode steps with.
        super().load_state_dict(state_dict)
        # torch casts every floating-point state tensor to the parameter's
        # dtype; the moments and the master copy of a bf16 parameter are fp32
        saved_ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        own = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(saved_ids, own):
            for key in ("exp_avg", "exp_avg_sq", "master"):
                saved = state_dict["state"].get(i, {}).get(key)
                if saved is not None:
                    self.state[p][key] = saved.detach().to(
                        device=_local_view(p).device, dtype=torch.float32, copy=True)
        for p, state in self.state.items():
            if "step" not in state:
                continue
            step = state["step"]
            if self.max_grad_norm is not None:
                dev = _local_view(p).device
                state["step"] = torch.as_tensor(step).to(
                    device=dev, dtype=torch.int32).reshape(()).clone()
            elif isinstance(step, torch.Tensor):
                state["step"] = int(step.item())

    def _stream_ids(self) -> Dict[torch.Tensor, int]:
        """Every parameter's index in the flattened ``param_groups`` order, the
        number ``state_dict()`` knows it by: its stream of random bits. Empty
        unless the mode is stochastic."""
        if self.rounding != "stochastic":
            return {}
        flat = (p for g in self.param_groups for p in g["params"])
        return {p: i for i, p in enumerate(flat)}

    def _gather(self, group: dict, all_ids: Dict[torch.Tensor, int]) -> _Rows:
        """The rows of one param group's parameters that have a gradient; their
        state is created on first sight."""
        clip = self.max_grad_norm is not None
        master, stochastic = self.rounding == "master", self.rounding == "stochastic"
        rows = _Rows(*([] for _ in _Rows._fields))
        params, grads, exp_avgs, exp_avg_sqs, steps, masters, stream_ids, states = rows
        for p in group["params"]:
            if p.grad is None:
                continue
            state = self.state[p]
            p_loc = _local_view(p)
            if len(state) == 0:
                # in clip mode the step lives on the device: a skipped step must
                # not advance it, and the host never learns which were skipped
                state["step"] = (torch.zeros((), dtype=torch.int32, device=p_loc.device)
                                 if clip else 0)
                state["exp_avg"] = torch.zeros_like(p_loc, dtype=torch.float32)
                state["exp_avg_sq"] = torch.zeros_like(p_loc, dtype=torch.float32)
            if master:
                if "master" not in state:
                    state["master"] = p_loc.float().contiguous()
                masters.append(state["master"])
            elif stochastic:
                stream_ids.append(all_ids[p])
            params.append(p_loc)
            grads.append(_local_view(p.grad))
            exp_avgs.append(state["exp_avg"])
            exp_avg_sqs.append(state["exp_avg_sq"])
            steps.append(state["step"])
            states.append(state)
        return rows

    def _ext_args(self, rows: _Rows, **seeds) -> dict:
        """The trailing arguments of ``adamw_step`` (``sr_seed=``) and
        ``adamw_clip_step`` (``sr_seeds=``); the seeds go with stochastic."""
        if self.rounding == "master":
            return dict(rounding=2, masters=rows.masters)
        if self.rounding == "stochastic":
            return dict(rounding=1, stream_ids=rows.stream_ids, **seeds)
        return {}

    def _torch_step(self, group: dict, rows: _Rows, j: int, bc1, bc2, step,
                    coef=None, finite=None) -> None:
        """The plain-torch update of row ``j``, taking step count ``step`` with
        the bias corrections ``bc1`` / ``bc2``. The clip mode gives ``coef`` and
        ``finite`` (0-dim device tensors) and, with no host sync, every tensor
        is rewritten through where(finite, new, old)."""
        p, g, m, v = rows.params[j], rows.grads[j], rows.exp_avgs[j], rows.exp_avg_sqs[j]
        master = rows.masters[j] if rows.masters else None
        beta1, beta2 = group["betas"]
        lr, wd = group["lr"], group["weight_decay"]

        def store(dst: torch.Tensor, new: torch.Tensor) -> None:
            dst.copy_(new if finite is None else torch.where(finite, new, dst))

        # The one place the modes differ in arithmetic, kept as each was: torch
        # evaluates the in-place forms with a fused multiply-add on the CPU, the
        # out-of-place ones round every product, and the last bit of about one
        # element in ten depends on it.
        if finite is None:
            gf = g.float()
            m_new = m.mul_(beta1).add_(gf, alpha=1 - beta1)
            v_new = v.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
        else:
            gf = g.float() * coef
            m_new = m * beta1 + gf * (1 - beta1)
            v_new = v * beta2 + gf * gf * (1 - beta2)
        denom = (v_new / bc2).sqrt_().add_(group["eps"])
        if self.rounding == "nearest":
            # rounds the update to p's dtype and adds there: two roundings
            update = (m_new / bc1) / denom + wd * p.float()
            p_new = p + (-lr * update).to(p.dtype)
        else:
            # starts from the master copy wherever its rounding still has the
            # bits of p, else from p, which someone has written since
            start = p.float()
            if master is not None:
                as_int = {2: torch.int16, 4: torch.int32, 8: torch.int64}[p.element_size()]
                ours = master.to(p.dtype).view(as_int) == p.view(as_int)
                start = torch.where(ours, master, start)
            update = (m_new / bc1) / denom + wd * start
            new32 = start - lr * update
            if master is not None:
                store(master, new32)
            if self.rounding == "stochastic" and p.dtype == torch.bfloat16:
                # the bits need the step count on the host: in clip mode, where
                # it is a device tensor, this path syncs
                r16 = sr_bits(p.numel(), seed=int(group.get("sr_seed", 0)), step=int(step),
                              stream_id=rows.stream_ids[j])
                p_new = stochastic_round_bf16(new32.reshape(-1), r16.to(p.device)).view_as(p)
            else:
                p_new = new32.to(p.dtype)
        store(p, p_new)
        if finite is not None:
            store(m, m_new)
            store(v, v_new)

    @torch.no_grad()
    def _step_clip(self) -> None:
        all_ids = self._stream_ids()
        groups = self.param_groups
        per_group = [self._gather(group, all_ids) for group in groups]
        rows = _Rows(*(sum(cols, []) for cols in zip(*per_group)))
        params, grads = rows.params, rows.grads
        if not params:
            return
        dev = params[0].device
        if self._sumsq.device != dev:
            self._clip_buffers(dev)

        if dev.type == "cuda" and all(
            p.dtype == torch.bfloat16 and g.dtype == torch.bfloat16
            for p, g in zip(params, grads)
        ):
            # norm over everything, then one update launch per param group —
            # no bucketing by step count, the kernel reads each tensor's own
            hip_ext().adamw_clip_step(
                params, grads, rows.exp_avgs, rows.exp_avg_sqs, rows.steps,
                [len(r.params) for r in per_group],
                [float(g["lr"]) for g in groups],
                [float(g["betas"][0]) for g in groups],
                [float(g["betas"][1]) for g in groups],
                [float(g["eps"]) for g in groups],
                [float(g["weight_decay"]) for g in groups],
                self.max_grad_norm, 2048, self._sumsq, self.skipped_steps,
                self.last_grad_norm, self.norm_reduce,
                **self._ext_args(rows, sr_seeds=[int(g.get("sr_seed", 0)) for g in groups]),
            )
            return

        # plain-torch path, same semantics and still no host sync
        self._sumsq.copy_(_sumsq_torch(grads))
        if self.norm_reduce is not None:
            self.norm_reduce(self._sumsq)
        norm = self._sumsq.sqrt().reshape(())
        finite = torch.isfinite(norm)
        coef = (self.max_grad_norm / (norm + 1e-6)).clamp(max=1.0)
        for group, own in zip(groups, per_group):
            beta1, beta2 = group["betas"]
            for j, s in enumerate(own.steps):
                taking = s + 1
                s1 = taking.double()
                self._torch_step(group, own, j, (1 - beta1 ** s1).float(),
                                 (1 - beta2 ** s1).float(), taking, coef, finite)
                s.add_(finite.to(s.dtype))
        self.last_grad_norm.copy_(norm)
        self.skipped_steps.add_((~finite).to(torch.int32))

    @torch.no_grad()
    def step(self, closure=None):  # noqa: D102
        assert closure is None
        if self.max_grad_norm is not None:
            self._step_clip()
            return None
        all_ids = self._stream_ids()
        for group in self.param_groups:
            rows = self._gather(group, all_ids)
            # Params that intermittently have grad=None (e.g. unused-param
            # DDP) accumulate different step counts; the bias correction is
            # per step count, so bucket by it — one kernel launch per
            # distinct count (one in the common case).
            by_step: Dict[int, List[int]] = {}
            for j, (state, step) in enumerate(zip(rows.states, rows.steps)):
                state["step"] = step = step + 1
                by_step.setdefault(step, []).append(j)

            beta1, beta2 = group["betas"]
            for step, idx in by_step.items():
                bucket = rows if len(idx) == len(rows.params) else rows.pick(idx)
                params = bucket.params
                if params[0].is_cuda and params[0].dtype == torch.bfloat16:
                    hip_ext().adamw_step(
                        params, bucket.grads, bucket.exp_avgs, bucket.exp_avg_sqs,
                        group["lr"], beta1, beta2, group["eps"], group["weight_decay"], step,
                        **self._ext_args(bucket, sr_seed=int(group.get("sr_seed", 0))),
                    )
                else:
                    for j in range(len(params)):
                        self._torch_step(group, bucket, j, 1 - beta1**step,
                                         1 - beta2**step, step)
        return None
