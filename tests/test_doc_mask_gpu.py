"""Document-masked causal attention on the GPU: the DOC variants of the
forward, dkdv and dq kernels against dense-mask attention in fp64, the
single-document case bit for bit against the unmasked kernels, no leak across
a boundary, determinism, what the bindings refuse, and the autograd path."""

import functools

import pytest
import torch

from attention_check import DOC_LAYOUTS as LAYOUTS, doc_mask as _mask

pytestmark = pytest.mark.gpu

D = 128
SCALE = D ** -0.5
# loose absolute tolerances shared with tests/test_flash_attn_gpu.py; the
# derived bounds for two of these layouts: tests/test_flash_attn_numerics_gpu.py
TOL_OUT, TOL_LSE, TOL_GRAD = 2e-2, 1e-3, 5e-2

HEADS = [(2, 2), (8, 2)]


def _ext():
    from torchft_amd.ops import hip_ext

    return hip_ext()


def _close(what, got, ref, tol):
    diff = (got.double() - ref.double()).abs()
    ratio = (diff / (tol + tol * ref.double().abs())).max().item()
    print(f"{what}: max abs err {diff.max().item():.3e}, worst ratio {ratio:.3f} "
          f"of rtol = atol = {tol:g}")
    torch.testing.assert_close(got.double(), ref.double(), rtol=tol, atol=tol)


def _reference(q, k, v, dout, dense):
    """Dense-mask attention in fp64 from the bf16 inputs, with autograd."""
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    G = q.shape[1] // k.shape[1]
    s = (qd @ kd.repeat_interleave(G, dim=1).transpose(-1, -2)) * SCALE
    s = s.masked_fill(~dense, float("-inf"))
    out = torch.softmax(s, dim=-1) @ vd.repeat_interleave(G, dim=1)
    out.backward(dout.double())
    return dict(out=out.detach(), lse=torch.logsumexp(s.detach(), dim=-1),
                dq=qd.grad, dk=kd.grad, dv=vd.grad)


@functools.lru_cache(maxsize=None)
def _case(name, Hq, Hkv):
    """Inputs as [B,S,H,D]-backed views, the mask and the fp64 reference,
    computed once per (layout, heads) and left unchanged."""
    S, rows = LAYOUTS[name]
    B = len(rows)
    g = torch.Generator(device="cuda").manual_seed(41)

    def mk(H):
        return torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16,
                           generator=g).transpose(1, 2)

    q, k, v, dout = mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)
    m = _mask(name)
    return q, k, v, dout, m, _reference(q, k, v, dout, m.dense())


def _run(q, k, v, dout, m):
    """The three DOC kernels as the autograd path chains them."""
    ext = _ext()
    out, lse = ext.fa_fwd(q, k, v, SCALE, True, m.doc_start, m.doc_end)
    delta = ext.fa_delta(dout, out)
    dq, dk, dv = ext.fa_bwd(q, k, v, dout, lse, delta, SCALE, True,
                            m.doc_start, m.doc_end)
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)


def _check(got, ref, rows=slice(None)):
    _close("out", got["out"][:, :, rows], ref["out"][:, :, rows], TOL_OUT)
    _close("lse", got["lse"][:, :, rows], ref["lse"][:, :, rows], TOL_LSE)
    for n in ("dq", "dk", "dv"):
        _close(n, got[n][:, :, rows], ref[n][:, :, rows], TOL_GRAD)


class TestAgainstReference:
    @pytest.mark.parametrize("packed", [False, True], ids=["bshd", "packed"])
    @pytest.mark.parametrize("Hq,Hkv", HEADS)
    @pytest.mark.parametrize("name", list(LAYOUTS))
    def test_fwd_bwd(self, name, Hq, Hkv, packed):
        q, k, v, dout, m, ref = _case(name, Hq, Hkv)
        if packed:
            q, k, v, dout = (t.contiguous() for t in (q, k, v, dout))
        got = _run(q, k, v, dout, m)
        assert got["out"].is_contiguous() == packed
        _check(got, ref)

    @pytest.mark.parametrize("name", ["mixed256", "halves512"])
    def test_layouts_agree_bitwise_and_calls_repeat(self, name):
        """Packed and [B,S,H,D] storage give the same bits, and so do two
        identical calls."""
        q, k, v, dout, m, _ = _case(name, 8, 2)
        a = _run(q, k, v, dout, m)
        b = _run(q, k, v, dout, m)
        c = _run(*(t.contiguous() for t in (q, k, v, dout)), m)
        for n in a:
            assert torch.equal(a[n], b[n]), n
            assert torch.equal(a[n], c[n]), n


class TestSingleDocument:
    @pytest.mark.parametrize("packed", [False, True], ids=["bshd", "packed"])
    @pytest.mark.parametrize("Hq,Hkv", HEADS)
    @pytest.mark.parametrize("S", [256, 512])
    def test_equals_plain_causal_bitwise(self, S, Hq, Hkv, packed):
        """doc_start = 0 and doc_end = S everywhere: the masks coincide and no
        tile is skipped, so the arithmetic is the causal kernels'."""
        from torchft_amd.ops import DocMask

        q, k, v, dout, _, _ = _case("mixed256" if S == 256 else "halves512", Hq, Hkv)
        if packed:
            q, k, v, dout = (t.contiguous() for t in (q, k, v, dout))
        m = DocMask.from_lengths([[S], [S]], S, device="cuda")
        assert int(m.doc_start.max()) == 0 and int(m.doc_end.min()) == S
        ext = _ext()
        got = _run(q, k, v, dout, m)
        out, lse = ext.fa_fwd(q, k, v, SCALE, True)
        dq, dk, dv = ext.fa_bwd(q, k, v, dout, lse, ext.fa_delta(dout, out), SCALE, True)
        for n, t in dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv).items():
            assert torch.equal(got[n], t), n


class TestNoLeak:
    """Scaling one side of a document boundary by 50 must not reach the other
    side. `cut` is a boundary in both rows of the layout."""

    @pytest.mark.parametrize("S,rows,cut", [
        (256, ([37, 219], [5, 32, 219]), 37),        # inside wave 1
        (512, ([300, 212], [100, 200, 212]), 300),   # inside the second workgroup
    ], ids=["cut37_256", "cut300_512"])
    @pytest.mark.parametrize("perturb_second", [True, False], ids=["second", "first"])
    def test_backward_bitwise_forward_within_tolerance(self, S, rows, cut, perturb_second):
        from torchft_amd.ops import DocMask

        assert all(cut in _cuts(r) for r in rows)
        Hq, Hkv = 8, 2
        g = torch.Generator(device="cuda").manual_seed(43)

        def mk(H):
            return torch.randn(2, S, H, D, device="cuda", dtype=torch.bfloat16,
                               generator=g).transpose(1, 2)

        q, k, v, dout = mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)
        m = DocMask.from_lengths(rows, S, device="cuda")
        ext = _ext()
        out, lse = ext.fa_fwd(q, k, v, SCALE, True, m.doc_start, m.doc_end)
        delta = ext.fa_delta(dout, out)
        base = ext.fa_bwd(q, k, v, dout, lse, delta, SCALE, True, m.doc_start, m.doc_end)

        hit = slice(cut, S) if perturb_second else slice(0, cut)
        keep = slice(0, cut) if perturb_second else slice(cut, S)

        def scaled(t):
            t = t.clone()  # keeps the [B,S,H,D] strides
            t[:, :, hit] *= 50
            return t

        q2, k2, v2, dout2 = scaled(q), scaled(k), scaled(v), scaled(dout)
        # fixed lse and delta: only the masked products could carry the change
        again = ext.fa_bwd(q2, k2, v2, dout2, lse, delta, SCALE, True,
                           m.doc_start, m.doc_end)
        for n, a, b_ in zip(("dq", "dk", "dv"), base, again):
            assert torch.equal(a[:, :, keep], b_[:, :, keep]), n
            assert not torch.equal(a[:, :, hit], b_[:, :, hit]), n

        # the forward's wave-wide defer-max decision couples rows, so its kept
        # side is held to the reference at the kernels' tolerances
        out2, lse2 = ext.fa_fwd(q2, k2, v2, SCALE, True, m.doc_start, m.doc_end)
        ref = _reference(q, k, v, dout, m.dense())
        _close("out", out2[:, :, keep], ref["out"][:, :, keep], TOL_OUT)
        _close("lse", lse2[:, :, keep], ref["lse"][:, :, keep], TOL_LSE)


def _cuts(row):
    at, c = 0, set()
    for n in row[:-1]:
        at += n
        c.add(at)
    return c


class TestRefusals:
    """The bindings refuse a bad mask before anything is launched."""

    B, Hq, Hkv, S = 2, 2, 1, 256

    def _good(self):
        def mk(*shape, dtype=torch.bfloat16):
            return torch.zeros(*shape, device="cuda", dtype=dtype)

        return dict(
            q=mk(self.B, self.Hq, self.S, D), k=mk(self.B, self.Hkv, self.S, D),
            v=mk(self.B, self.Hkv, self.S, D), dout=mk(self.B, self.Hq, self.S, D),
            lse=mk(self.B, self.Hq, self.S, dtype=torch.float32),
            delta=mk(self.B, self.Hq, self.S, dtype=torch.float32),
            doc_start=mk(self.B, self.S, dtype=torch.int32),
            doc_end=torch.full((self.B, self.S), self.S, device="cuda", dtype=torch.int32),
            causal=True,
        )

    def _fwd(self, a):
        return _ext().fa_fwd(a["q"], a["k"], a["v"], SCALE, a["causal"],
                             a["doc_start"], a["doc_end"])

    def _bwd(self, a):
        return _ext().fa_bwd(a["q"], a["k"], a["v"], a["dout"], a["lse"], a["delta"],
                             SCALE, a["causal"], a["doc_start"], a["doc_end"])

    def test_good_arguments_pass(self):
        a = self._good()
        self._fwd(a)
        self._bwd(a)
        # keywords, and a [B*S] shape with the right element count
        a["doc_start"] = a["doc_start"].reshape(-1)
        _ext().fa_fwd(a["q"], a["k"], a["v"], SCALE, True, doc_start=a["doc_start"],
                      doc_end=a["doc_end"])
        torch.cuda.synchronize()

    @pytest.mark.parametrize("call", ["_fwd", "_bwd"])
    @pytest.mark.parametrize("which", ["doc_start", "doc_end"])
    def test_int64(self, call, which):
        a = self._good()
        a[which] = a[which].long()
        with pytest.raises(RuntimeError, match=rf"fa_(fwd|bwd): {which} must be an int32"):
            getattr(self, call)(a)

    @pytest.mark.parametrize("call", ["_fwd", "_bwd"])
    @pytest.mark.parametrize("which", ["doc_start", "doc_end"])
    def test_twice_the_elements(self, call, which):
        a = self._good()
        a[which] = torch.zeros(self.B, 2 * self.S, device="cuda", dtype=torch.int32)
        with pytest.raises(RuntimeError, match=rf"fa_(fwd|bwd): {which} shape mismatch"):
            getattr(self, call)(a)

    @pytest.mark.parametrize("call", ["_fwd", "_bwd"])
    @pytest.mark.parametrize("which", ["doc_start", "doc_end"])
    def test_host_tensor(self, call, which):
        a = self._good()
        a[which] = a[which].cpu()
        with pytest.raises(RuntimeError, match=rf"fa_(fwd|bwd): {which} must be on q's device"):
            getattr(self, call)(a)

    @pytest.mark.parametrize("call", ["_fwd", "_bwd"])
    @pytest.mark.parametrize("which", ["doc_start", "doc_end"])
    def test_one_without_the_other(self, call, which):
        a = self._good()
        a[which] = None
        with pytest.raises(RuntimeError, match=rf"fa_(fwd|bwd): {which} is missing"):
            getattr(self, call)(a)

    @pytest.mark.parametrize("call", ["_fwd", "_bwd"])
    def test_mask_without_causal(self, call):
        a = self._good()
        a["causal"] = False
        with pytest.raises(RuntimeError, match=r"fa_(fwd|bwd): doc_start / doc_end need causal"):
            getattr(self, call)(a)


class TestEndToEnd:
    def test_autograd_through_views_takes_the_custom_forward(self, monkeypatch):
        """flash_attention with a mask runs the hand-written forward without
        TORCHFT_AMD_CUSTOM_FA_FWD, and the hand-written backward."""
        from torchft_amd.ops import flash_attention

        monkeypatch.delenv("TORCHFT_AMD_CUSTOM_FA_FWD", raising=False)
        monkeypatch.setenv("TORCHFT_AMD_CUSTOM_FA", "1")
        ext = _ext()
        calls = []
        real_fwd, real_bwd = ext.fa_fwd, ext.fa_bwd
        monkeypatch.setattr(ext, "fa_fwd", lambda *a, **kw: (
            calls.append(("fwd", len(a))), real_fwd(*a, **kw))[1])
        monkeypatch.setattr(ext, "fa_bwd", lambda *a, **kw: (
            calls.append(("bwd", len(a))), real_bwd(*a, **kw))[1])

        q0, k0, v0, dout, m, ref = _case("eighths512", 8, 2)
        # leaves in the projection layout, seen through transpose views
        leaves = [t.transpose(1, 2).contiguous().requires_grad_(True) for t in (q0, k0, v0)]
        out = flash_attention(*(t.transpose(1, 2) for t in leaves), causal=True, doc_mask=m)
        out.backward(dout)
        assert calls == [("fwd", 7), ("bwd", 10)]
        assert not out.is_contiguous()
        _close("out", out, ref["out"], TOL_OUT)
        for t, n in zip(leaves, ("dq", "dk", "dv")):
            _close(n, t.grad.transpose(1, 2), ref[n], TOL_GRAD)

    def test_disabled_custom_fa_falls_back_to_the_dense_mask(self, monkeypatch):
        from torchft_amd.ops import flash_attention

        monkeypatch.setenv("TORCHFT_AMD_CUSTOM_FA", "0")
        q, k, v, _, m, ref = _case("mixed256", 2, 2)
        out = flash_attention(q, k, v, causal=True, doc_mask=m)
        _close("out", out, ref["out"], TOL_OUT)

    def test_model_trains_with_the_mask(self, monkeypatch):
        """A head_dim-128 Llama with activation checkpointing: the masked loss
        through the kernels matches the dense-mask fallback (both bf16; the
        attention tolerances of the project bound the difference)."""
        from torchft_amd.models.llama import Llama, LlamaConfig
        from torchft_amd.ops import DocMask

        cfg = LlamaConfig(dim=256, n_layers=2, n_heads=2, n_kv_heads=1, ffn_hidden=512,
                          vocab_size=512, max_seq_len=256)
        torch.manual_seed(44)
        model = Llama(cfg, dtype=torch.bfloat16, checkpoint_activations=True).cuda().train()
        toks = torch.randint(0, cfg.vocab_size, (2, 257), device="cuda")
        m = DocMask.from_eos(torch.where(
            torch.arange(256, device="cuda") % 100 == 99, 1, 0).expand(2, 256), 1)
        assert m.doc_start[0, 255].item() == 200

        def loss_and_grad():
            model.zero_grad()
            loss = model.forward_loss(toks[:, :-1], toks[:, 1:], doc_mask=m)
            loss.backward()
            return loss.item(), model.layers[0].attn.wqkv.weight.grad.clone()

        def rel(a, b):
            return ((a.double() - b.double()).norm() / b.double().norm()).item()

        monkeypatch.setenv("TORCHFT_AMD_CUSTOM_FA", "1")
        loss_k, grad_k = loss_and_grad()
        model.zero_grad()
        model.forward_loss(toks[:, :-1], toks[:, 1:]).backward()
        grad_plain = model.layers[0].attn.wqkv.weight.grad.clone()
        monkeypatch.setenv("TORCHFT_AMD_CUSTOM_FA", "0")
        loss_f, grad_f = loss_and_grad()
        print(f"loss kernels {loss_k} fallback {loss_f}; wqkv.grad relative L2: "
              f"kernels vs fallback {rel(grad_k, grad_f):.3e}, "
              f"unmasked vs fallback {rel(grad_plain, grad_f):.3e}")
        assert loss_k == pytest.approx(loss_f, rel=TOL_OUT)
        assert torch.isfinite(grad_k).all()
        # two bf16 routes to one gradient: the kernels' gradient tolerance,
        # taken as a relative L2 distance; the unmasked gradient is another one
        assert rel(grad_k, grad_f) < TOL_GRAD
        assert rel(grad_plain, grad_f) > 2 * TOL_GRAD
