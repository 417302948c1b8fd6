"""GPU tests of the fused QKV split + rotary kernels (csrc/kernels/qkv_rope.hip,
the qkv_rope_fwd / qkv_rope_bwd bindings, ops.qkv_rope) and of the model path
built on them: bit equality with rope_apply on contiguous slices, forward and
backward, with and without per-token positions; the fp64 bound of the rotation;
the autograd path against the unfused composition; layouts, empty inputs and
refusals; and the Llama model with the fused path on and off."""

import dataclasses
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda:0"

# (B, S, Hq, Hkv, D)
SHAPES = [
    (1, 3, 2, 1, 16),      # one item per head; the table has more rows than S
    (2, 5, 4, 2, 128),
    (1, 130, 8, 2, 64),    # crosses a workgroup
    (2, 7, 3, 3, 128),     # Hq = Hkv and odd
    (1, 257, 32, 8, 128),  # the model's head counts
]
IDS = ["x".join(map(str, s)) for s in SHAPES]
EXTRA_ROWS = 3  # table rows beyond S


def _ext():
    from torchft_amd.ops import hip_ext

    return hip_ext()


def _randn(*shape, seed, dtype=BF16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, dtype=torch.float32, generator=g).to(dtype)


def _doc_positions(B, S):
    """DocMask.positions() of a layout with a boundary at 1 and at S - 1 in
    row 0 and, if there is one, two halves in row 1."""
    from torchft_amd.ops import DocMask

    rows = [[1, S - 2, 1]] + [[S // 2, S - S // 2]] * (B - 1)
    return DocMask.from_lengths(rows, S, device=DEV).positions()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs of one shape and the unfused results, computed once and left
    unchanged: rope_apply on contiguous slices (forward), on dq / dk
    (backward), each with global positions, random positions and a DocMask
    layout's positions (the gathered tables, one batch row at a time)."""
    from torchft_amd.ops import rope_tables

    ext = _ext()
    B, S, Hq, Hkv, D = shape
    W = (Hq + 2 * Hkv) * D
    rows = S + EXTRA_ROWS
    cos, sin = rope_tables(rows, D, device=DEV)
    qkv = _randn(B, S, W, seed=21)
    d = [_randn(B, S, h, D, seed=22 + i) for i, h in enumerate((Hq, Hkv, Hkv))]
    g = torch.Generator(device=DEV).manual_seed(25)
    positions = {
        "global": None,
        "random": torch.randint(0, rows, (B, S), device=DEV, dtype=torch.int32, generator=g),
        "docs": _doc_positions(B, S),
    }
    nq, nkv = Hq * D, Hkv * D
    parts = [qkv[..., :nq].view(B, S, Hq, D), qkv[..., nq:nq + nkv].view(B, S, Hkv, D),
             qkv[..., nq + nkv:].view(B, S, Hkv, D)]

    def unfused(x, pos, backward):
        x = x.contiguous()
        if pos is None:
            return ext.rope_apply(x, cos, sin, backward)
        return torch.cat([
            ext.rope_apply(x[b:b + 1].contiguous(), cos[pos[b].long()], sin[pos[b].long()],
                           backward) for b in range(B)])

    ref = {}
    for name, pos in positions.items():
        fwd = [unfused(parts[0], pos, False), unfused(parts[1], pos, False),
               parts[2].contiguous()]
        bwd = torch.cat([unfused(d[0], pos, True).reshape(B, S, -1),
                         unfused(d[1], pos, True).reshape(B, S, -1),
                         d[2].reshape(B, S, -1)], -1)
        ref[name] = (fwd, bwd)
    return dict(qkv=qkv, d=d, cos=cos, sin=sin, positions=positions, ref=ref, parts=parts)


@pytest.mark.parametrize("which", ["global", "random", "docs"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
class TestEqualsRopeApply:
    def test_forward(self, shape, which):
        B, S, Hq, Hkv, D = shape
        c = _case(shape)
        q, k, v = _ext().qkv_rope_fwd(c["qkv"], c["cos"], c["sin"], Hq, Hkv,
                                      c["positions"][which])
        for got, want, h in zip((q, k, v), c["ref"][which][0], (Hq, Hkv, Hkv)):
            assert got.shape == (B, S, h, D) and got.dtype == BF16 and got.is_contiguous()
            assert torch.equal(got, want)

    def test_backward(self, shape, which):
        """Every element of dqkv: the output was never zero-filled."""
        B, S, Hq, Hkv, D = shape
        c = _case(shape)
        dqkv = _ext().qkv_rope_bwd(*c["d"], c["cos"], c["sin"], c["positions"][which])
        assert dqkv.shape == (B, S, (Hq + 2 * Hkv) * D) and dqkv.is_contiguous()
        assert torch.equal(dqkv, c["ref"][which][1])


def _rotate_fp64(x, cos, sin, pos, sign):
    """The rotation of [B, S, H, D] in fp64 and the bound of its fp32
    evaluation: the result and |x1||c| + |x2||s| per element."""
    B, S, _, D = x.shape
    idx = pos.long() if pos is not None else torch.arange(S, device=x.device).expand(B, S)
    c = cos.double()[idx].view(B, S, 1, D // 2)
    s = sin.double()[idx].view(B, S, 1, D // 2) * sign
    x1, x2 = x.double().chunk(2, dim=-1)
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    mag = torch.cat([x1.abs() * c.abs() + x2.abs() * s.abs(),
                     x2.abs() * c.abs() + x1.abs() * s.abs()], -1)
    return out, mag


@pytest.mark.parametrize("which", ["global", "random"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fp64_bound(shape, which):
    """q, k and the rotated part of dqkv against the rotation in fp64 from the
    same bf16 inputs and fp32 tables: (u + 3e) * (|x1||c| + |x2||s|) per
    element, u = 2^-8 for the one bf16 store, e = 2^-24 for each of the two
    products and the sum in fp32. Worst fraction of the bound over the five
    shapes: see docs/KERNELS.md, "qkv_rope.hip"."""
    B, S, Hq, Hkv, D = shape
    c = _case(shape)
    pos = c["positions"][which]
    ext = _ext()
    q, k, _ = ext.qkv_rope_fwd(c["qkv"], c["cos"], c["sin"], Hq, Hkv, pos)
    dqkv = ext.qkv_rope_bwd(*c["d"], c["cos"], c["sin"], pos)
    nq, nkv = Hq * D, Hkv * D
    pairs = [
        ("q", q, c["parts"][0], 1.0),
        ("k", k, c["parts"][1], 1.0),
        ("dqkv[q]", dqkv[..., :nq].reshape(B, S, Hq, D), c["d"][0], -1.0),
        ("dqkv[k]", dqkv[..., nq:nq + nkv].reshape(B, S, Hkv, D), c["d"][1], -1.0),
    ]
    u, e = 2.0 ** -8, 2.0 ** -24
    for name, got, x, sign in pairs:
        want, mag = _rotate_fp64(x, c["cos"], c["sin"], pos, sign)
        err = (got.double() - want).abs()
        bound = (u + 3 * e) * mag
        frac = (err / bound.clamp_min(1e-300)).max().item()
        print(f"{name} {shape} {which}: worst error / bound {frac:.4f}")
        assert torch.all(err <= bound), name


@pytest.mark.parametrize("which", ["global", "docs"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_autograd_equals_the_unfused_composition(shape, which):
    from torchft_amd.ops import qkv_rope, rope

    B, S, Hq, Hkv, D = shape
    c = _case(shape)
    pos = c["positions"][which]
    cos, sin = c["cos"], c["sin"]
    # one gradient arrives as a transposed view, as attention's do
    douts = [_randn(B, Hq, S, D, seed=31).transpose(1, 2), c["d"][1], c["d"][2]]
    assert not douts[0].is_contiguous()

    def unfused(qkv):
        nq, nkv = Hq * D, Hkv * D
        q = qkv[..., :nq].view(B, S, Hq, D)
        k = qkv[..., nq:nq + nkv].view(B, S, Hkv, D)
        v = qkv[..., nq + nkv:].view(B, S, Hkv, D)
        if pos is None:
            return rope(q, cos, sin), rope(k, cos, sin), v
        rot = lambda x: torch.cat([  # noqa: E731
            rope(x[b:b + 1], cos[pos[b].long()], sin[pos[b].long()]) for b in range(B)])
        return rot(q), rot(k), v

    results = []
    for fn in (lambda t: qkv_rope(t, cos, sin, Hq, Hkv, pos), unfused):
        leaf = c["qkv"].detach().clone().requires_grad_(True)
        outs = fn(leaf)
        torch.autograd.backward(outs, douts)
        results.append(([o.detach() for o in outs], leaf.grad))
    (got, got_grad), (want, want_grad) = results
    for a, b_ in zip(got, want):
        assert torch.equal(a, b_)
    assert torch.equal(got_grad, want_grad)


def test_only_the_tables_and_positions_are_saved():
    from torchft_amd.ops import qkv_rope

    B, S, Hq, Hkv, D = SHAPES[1]
    c = _case(SHAPES[1])
    leaf = c["qkv"].detach().clone().requires_grad_(True)
    q, _, _ = qkv_rope(leaf, c["cos"], c["sin"], Hq, Hkv, c["positions"]["docs"])
    saved = [t for t in q.grad_fn.saved_tensors]
    assert {t.data_ptr() for t in saved} == {
        c["cos"].data_ptr(), c["sin"].data_ptr(), c["positions"]["docs"].data_ptr()}


class TestLayouts:
    SHAPE = SHAPES[1]

    def test_qkv_one_element_off_a_16_byte_boundary(self):
        B, S, Hq, Hkv, D = self.SHAPE
        c = _case(self.SHAPE)
        buf = torch.empty(c["qkv"].numel() + 1, device=DEV, dtype=BF16)
        view = buf[1:].view_as(c["qkv"])
        view.copy_(c["qkv"])
        assert view.data_ptr() % 16 == 2
        got = _ext().qkv_rope_fwd(view, c["cos"], c["sin"], Hq, Hkv)
        for a, b_ in zip(got, c["ref"]["global"][0]):
            assert torch.equal(a, b_)

    def test_dq_as_a_transpose_view(self):
        c = _case(self.SHAPE)
        dq = c["d"][0].transpose(1, 2).contiguous().transpose(1, 2)
        assert not dq.is_contiguous() and torch.equal(dq, c["d"][0])
        got = _ext().qkv_rope_bwd(dq, c["d"][1], c["d"][2], c["cos"], c["sin"])
        assert torch.equal(got, c["ref"]["global"][1])


@pytest.mark.parametrize("B,S", [(0, 5), (2, 0)])
def test_empty_inputs(B, S):
    from torchft_amd.ops import rope_tables

    Hq, Hkv, D = 4, 2, 32
    ext = _ext()
    cos, sin = rope_tables(8, D, device=DEV)
    qkv = torch.empty(B, S, (Hq + 2 * Hkv) * D, device=DEV, dtype=BF16)
    for pos in (None, torch.empty(B, S, device=DEV, dtype=torch.int32)):
        q, k, v = ext.qkv_rope_fwd(qkv, cos, sin, Hq, Hkv, pos)
        assert q.shape == (B, S, Hq, D) and k.shape == (B, S, Hkv, D) and v.shape == k.shape
        assert q.dtype == BF16 and q.device == qkv.device
        dqkv = ext.qkv_rope_bwd(q, k, v, cos, sin, pos)
        assert dqkv.shape == qkv.shape and dqkv.dtype == BF16
    torch.cuda.synchronize()


class TestRefusals:
    """Each refusal names the binding and the argument, before any launch."""

    B, S, Hq, Hkv, D = 2, 5, 4, 2, 32

    def _good(self):
        from torchft_amd.ops import rope_tables

        cos, sin = rope_tables(self.S, self.D, device=DEV)
        z = lambda *s, dtype=BF16: torch.zeros(*s, device=DEV, dtype=dtype)  # noqa: E731
        return dict(
            qkv=z(self.B, self.S, (self.Hq + 2 * self.Hkv) * self.D), cos=cos, sin=sin,
            positions=None, dq=z(self.B, self.S, self.Hq, self.D),
            dk=z(self.B, self.S, self.Hkv, self.D), dv=z(self.B, self.S, self.Hkv, self.D))

    def _fwd(self, a, Hq=None, Hkv=None):
        return _ext().qkv_rope_fwd(a["qkv"], a["cos"], a["sin"], Hq or self.Hq,
                                   Hkv or self.Hkv, a["positions"])

    def _bwd(self, a):
        return _ext().qkv_rope_bwd(a["dq"], a["dk"], a["dv"], a["cos"], a["sin"],
                                   a["positions"])

    def test_good_arguments_pass(self):
        a = self._good()
        self._fwd(a)
        self._bwd(a)
        # keywords; with positions one table row is enough
        a["positions"] = torch.zeros(self.B * self.S, device=DEV, dtype=torch.int32)
        _ext().qkv_rope_fwd(a["qkv"], a["cos"][:1], a["sin"][:1], n_heads=self.Hq,
                            n_kv_heads=self.Hkv, positions=a["positions"])
        _ext().qkv_rope_bwd(a["dq"], a["dk"], a["dv"], a["cos"][:1], a["sin"][:1],
                            positions=a["positions"])
        torch.cuda.synchronize()

    def test_fp16_qkv(self):
        a = self._good()
        a["qkv"] = a["qkv"].half()
        with pytest.raises(RuntimeError, match=r"qkv_rope_fwd: qkv must be BFloat16"):
            self._fwd(a)

    def test_width_not_divisible(self):
        a = self._good()
        with pytest.raises(RuntimeError, match=r"qkv_rope_fwd: the last dimension of qkv "
                                               r"\(W = 256\) must be divisible"):
            self._fwd(a, Hq=3)

    def test_head_dim_24(self):
        a = self._good()
        a["qkv"] = torch.zeros(self.B, self.S, 8 * 24, device=DEV, dtype=BF16)
        with pytest.raises(RuntimeError, match=r"qkv_rope_fwd: the head dimension of qkv "
                                               r"\(D\) must be a multiple of 16.*got 24"):
            self._fwd(a)

    def test_int64_positions(self):
        a = self._good()
        a["positions"] = torch.zeros(self.B, self.S, device=DEV, dtype=torch.int64)
        with pytest.raises(RuntimeError, match=r"qkv_rope_fwd: positions must be Int"):
            self._fwd(a)
        with pytest.raises(RuntimeError, match=r"qkv_rope_bwd: positions must be Int"):
            self._bwd(a)

    def test_positions_with_twice_the_elements(self):
        a = self._good()
        a["positions"] = torch.zeros(self.B, 2 * self.S, device=DEV, dtype=torch.int32)
        with pytest.raises(RuntimeError, match=r"qkv_rope_fwd: positions must have 10 "):
            self._fwd(a)
        with pytest.raises(RuntimeError, match=r"qkv_rope_bwd: positions must have 10 "):
            self._bwd(a)

    def test_host_positions(self):
        a = self._good()
        a["positions"] = torch.zeros(self.B, self.S, dtype=torch.int32)
        with pytest.raises(RuntimeError, match=r"qkv_rope_fwd: positions must be a device"):
            self._fwd(a)
        with pytest.raises(RuntimeError, match=r"qkv_rope_bwd: positions must be a device"):
            self._bwd(a)

    def test_sin_tab_of_another_shape(self):
        a = self._good()
        a["sin"] = torch.cat([a["sin"], a["sin"]])
        with pytest.raises(RuntimeError, match=r"qkv_rope_fwd: sin_tab must have the shape"):
            self._fwd(a)
        with pytest.raises(RuntimeError, match=r"qkv_rope_bwd: sin_tab must have the shape"):
            self._bwd(a)

    def test_short_tables_without_positions(self):
        a = self._good()
        a["cos"], a["sin"] = a["cos"][:self.S - 1], a["sin"][:self.S - 1]
        with pytest.raises(RuntimeError, match=r"qkv_rope_fwd: cos_tab must be \[at least 5"):
            self._fwd(a)
        with pytest.raises(RuntimeError, match=r"qkv_rope_bwd: cos_tab must be \[at least 5"):
            self._bwd(a)

    def test_dk_with_another_sequence_length(self):
        a = self._good()
        a["dk"] = torch.zeros(self.B, self.S + 1, self.Hkv, self.D, device=DEV, dtype=BF16)
        with pytest.raises(RuntimeError, match=r"qkv_rope_bwd: dk must be \[B, S, Hkv, D\]"):
            self._bwd(a)

    def test_dv_with_another_shape(self):
        a = self._good()
        a["dv"] = torch.zeros(self.B, self.S, self.Hkv + 1, self.D, device=DEV, dtype=BF16)
        with pytest.raises(RuntimeError, match=r"qkv_rope_bwd: dv must have the shape"):
            self._bwd(a)


# ---------------------------------------------------------------- the model


def _is_bshd(t):
    """bindings.cpp, is_bshd: a logical [B,H,S,D] tensor that is a transpose
    view of contiguous [B,S,H,D] storage."""
    return (t.dim() == 4 and t.stride(3) == 1 and t.stride(1) == t.size(3)
            and t.stride(2) == t.size(1) * t.size(3)
            and t.stride(0) == t.size(1) * t.size(2) * t.size(3))


class TestModel:
    """The config of test_doc_mask_gpu.py::test_model_trains_with_the_mask:
    head_dim 128, activation checkpointing on."""

    S = 256

    def _cfg(self, **kw):
        from torchft_amd.models.llama import LlamaConfig

        return LlamaConfig(dim=256, n_layers=2, n_heads=2, n_kv_heads=1, ffn_hidden=512,
                           vocab_size=512, max_seq_len=self.S, **kw)

    def _model(self, **kw):
        from torchft_amd.models.llama import Llama

        torch.manual_seed(44)
        return Llama(self._cfg(**kw), dtype=BF16, checkpoint_activations=True).cuda().train()

    def _batch(self):
        from torchft_amd.ops import DocMask

        g = torch.Generator(device=DEV).manual_seed(45)
        toks = torch.randint(0, 512, (2, self.S + 1), device=DEV, generator=g)
        mask = DocMask.from_lengths([[100, 156], [1, 254, 1]], self.S, device=DEV)
        return toks, mask

    @staticmethod
    def _step(model, toks, mask, fused_ce=False):
        model.zero_grad()
        loss = model.forward_loss(toks[:, :-1], toks[:, 1:], doc_mask=mask, fused=fused_ce)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}

    @pytest.mark.parametrize("masked", [False, True], ids=["causal", "doc_mask"])
    def test_fused_path_on_and_off_give_the_same_bits(self, monkeypatch, masked):
        """The loss and every parameter gradient, torch.equal.

        rmsnorm_bwd sums the weight gradient with fp32 atomics in whatever
        order its workgroups finish (docs/ROADMAP.md, item 12), so two
        IDENTICAL steps of this model, the flag at 0 both times, already
        differ in `norm.weight.grad` and `attn_norm.weight.grad` (measured on
        MI355X: 3 of 3 repeats with the mask). For this comparison both steps
        therefore take dw as a fixed-order torch sum of the same dy * x *
        invrms; dx stays the kernel's. The norm weights are still compared:
        their gradient now depends on nothing but the dy and x that reach the
        norms, which is where the flag could show."""
        ext = _ext()
        real_rmsnorm_bwd = ext.rmsnorm_bwd

        def rmsnorm_bwd_fixed_order(dy, x, w, invrms):
            dx, _ = real_rmsnorm_bwd(dy, x, w, invrms)
            H = x.shape[-1]
            dw = (dy.float() * x.float()).reshape(-1, H).mul_(invrms.reshape(-1, 1)).sum(0)
            return dx, dw

        monkeypatch.setattr(ext, "rmsnorm_bwd", rmsnorm_bwd_fixed_order)
        model = self._model()
        toks, mask = self._batch()
        mask = mask if masked else None
        monkeypatch.setenv("TORCHFT_AMD_FUSED_QKV_ROPE", "1")
        loss_on, grads_on = self._step(model, toks, mask)
        monkeypatch.setenv("TORCHFT_AMD_FUSED_QKV_ROPE", "0")
        loss_off, grads_off = self._step(model, toks, mask)
        assert torch.isfinite(loss_on) and torch.equal(loss_on, loss_off)
        # embedding, head, final norm and six tensors per layer
        assert grads_on.keys() == grads_off.keys() and len(grads_on) == 3 + 6 * 2
        differ = [n for n in grads_on if not torch.equal(grads_on[n], grads_off[n])]
        assert not differ, differ

    @pytest.mark.parametrize("masked", [False, True], ids=["causal", "doc_mask"])
    def test_attention_gets_three_bshd_tensors(self, monkeypatch, masked):
        """With the fused path q, k and v reach flash_attention as transpose
        views of contiguous [B,S,H,D] tensors, the layout the attention
        bindings take without a copy; with the flag off v is a slice of the
        projection and fails the stride test (which is what sent the whole
        call down the copying path)."""
        import torchft_amd.models.llama as llama

        seen = []
        real = llama.flash_attention

        def spy(q, k, v, **kw):
            seen.append([_is_bshd(t) for t in (q, k, v)])
            return real(q, k, v, **kw)

        monkeypatch.setattr(llama, "flash_attention", spy)
        model = self._model().eval()
        toks, mask = self._batch()
        mask = mask if masked else None
        with torch.no_grad():
            monkeypatch.setenv("TORCHFT_AMD_FUSED_QKV_ROPE", "1")
            model.forward_hidden(toks[:, :-1], doc_mask=mask)
            assert seen == [[True, True, True]] * 2
            seen.clear()
            monkeypatch.delenv("TORCHFT_AMD_FUSED_QKV_ROPE")
            model.forward_hidden(toks[:, :-1], doc_mask=mask)
            assert seen == [[True, True, True]] * 2  # the default
            seen.clear()
            monkeypatch.setenv("TORCHFT_AMD_FUSED_QKV_ROPE", "0")
            model.forward_hidden(toks[:, :-1], doc_mask=mask)
            assert seen == [[True, True, False]] * 2

    def test_position_reset_trains(self, monkeypatch):
        """rope_doc_reset with a two-document mask: a finite loss that differs
        from the global-position loss, and a backward; the fused kernel runs
        even with the flag off."""
        toks, _ = self._batch()
        from torchft_amd.ops import DocMask

        mask = DocMask.from_lengths([[100, 156], [200, 56]], self.S, device=DEV)
        calls = []
        ext = _ext()
        real = ext.qkv_rope_fwd
        monkeypatch.setattr(ext, "qkv_rope_fwd", lambda *a, **kw: (
            calls.append(a[5] is not None), real(*a, **kw))[1])
        monkeypatch.setenv("TORCHFT_AMD_FUSED_QKV_ROPE", "0")
        # the fp32 loss head: the unfused one sums the row losses in bf16, in
        # steps of 16 / 512 rows here, too coarse to tell two losses apart
        loss_reset, grads = self._step(self._model(rope_doc_reset=True), toks, mask, True)
        # forward and recomputation of two checkpointed layers, with positions
        assert calls == [True] * 4
        loss_global, _ = self._step(self._model(), toks, mask, True)
        assert calls == [True] * 4  # flag off, no positions: the unfused path
        print(f"loss with reset {loss_reset.item()}, global {loss_global.item()}")
        assert torch.isfinite(loss_reset) and torch.isfinite(loss_global)
        assert loss_reset.item() != loss_global.item()
        assert all(torch.isfinite(g).all() for g in grads.values())
        assert grads["layers.0.attn.wqkv.weight"].abs().max() > 0
