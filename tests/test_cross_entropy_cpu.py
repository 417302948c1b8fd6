"""CPU tests of the fused linear + cross-entropy head: the plain-torch
reference against torch's own cross-entropy, ``linear_cross_entropy``
against ``F.cross_entropy(F.linear(...))``, the bounded-memory contract
(nothing [rows, vocab]-sized saved for backward) and the Llama switch."""

import pytest
import torch
import torch.nn.functional as F

from torchft_amd.models.llama import LLAMA_DEBUG, Llama
from torchft_amd.ops import linear_cross_entropy
from torchft_amd.ops.cross_entropy import cross_entropy_ref, fused_cross_entropy_

IGNORE = -100


def _logits_targets(V, rows=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V, generator=g) * 4.0
    t = torch.randint(0, V, (rows,), generator=g)
    t[0] = 0
    t[1] = V - 1
    t[2] = IGNORE
    return x, t


class TestReference:
    @pytest.mark.parametrize("V", [40, 1003])
    def test_matches_torch_cross_entropy(self, V):
        x, t = _logits_targets(V)
        xa = x.clone().requires_grad_(True)
        ref = F.cross_entropy(xa, t, ignore_index=IGNORE, reduction="sum")
        ref.backward()
        loss, grad = cross_entropy_ref(x, t, ignore_index=IGNORE)
        assert loss.dtype == torch.float32 and loss.shape == (x.shape[0],)
        assert loss[2].item() == 0.0
        assert torch.count_nonzero(grad[2]).item() == 0
        torch.testing.assert_close(loss.sum(), ref.detach())
        torch.testing.assert_close(grad, xa.grad)

    @pytest.mark.parametrize("V", [40, 1003])
    def test_z_loss_matches_autograd(self, V):
        z = 1e-4
        x, t = _logits_targets(V, seed=1)
        xa = x.clone().requires_grad_(True)
        keep = t != IGNORE
        lse = torch.logsumexp(xa, dim=-1)
        xt = xa.gather(1, t.clamp(min=0).unsqueeze(1)).squeeze(1)
        ref = ((lse - xt + z * lse**2) * keep).sum()
        ref.backward()
        loss, grad = cross_entropy_ref(x, t, ignore_index=IGNORE, z_loss=z)
        torch.testing.assert_close(loss.sum(), ref.detach())
        torch.testing.assert_close(grad, xa.grad)

    def test_grad_scale_and_inplace_contract(self):
        x, t = _logits_targets(40, seed=2)
        loss, grad = cross_entropy_ref(x, t, grad_scale=0.25)
        _, grad1 = cross_entropy_ref(x, t)
        torch.testing.assert_close(grad, 0.25 * grad1)
        buf = x.clone()
        out = fused_cross_entropy_(buf, t, grad_scale=torch.tensor([0.25]))
        torch.testing.assert_close(out, loss)
        torch.testing.assert_close(buf, grad)
        buf = x.clone()
        out = fused_cross_entropy_(buf, t, write_grad=False)
        assert torch.equal(buf, x)
        torch.testing.assert_close(out, loss)

    def test_out_of_range_target_is_loud(self):
        x, t = _logits_targets(40, seed=3)
        t[3] = 40
        loss, grad = cross_entropy_ref(x, t)
        assert torch.isnan(loss[3]) and torch.isnan(grad[3]).all()
        keep = torch.arange(x.shape[0]) != 3
        assert torch.isfinite(loss[keep]).all() and torch.isfinite(grad[keep]).all()

    def test_masked_vocab_and_large_logits(self):
        x, t = _logits_targets(40, seed=4)
        x = x * 750.0
        x[4, 5:30] = float("-inf")
        t[4] = 2
        for z in (0.0, 1e-4):
            loss, grad = cross_entropy_ref(x, t, z_loss=z)
            assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
            assert torch.count_nonzero(grad[4, 5:30]).item() == 0


N, D, V = 50, 32, 1003


def _head_inputs(seed=0, ignore_some=True):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(N, D, generator=g)
    w = torch.randn(V, D, generator=g) * 0.2
    t = torch.randint(0, V, (N,), generator=g)
    t[0] = 0
    t[1] = V - 1
    if ignore_some:
        t[2] = IGNORE
        t[N - 1] = IGNORE
    return h, w, t


def _torch_head(h, w, t, scale=1.0, h_grad=True):
    hr = h.clone().requires_grad_(h_grad)
    wr = w.clone().requires_grad_(True)
    loss = F.cross_entropy(F.linear(hr, wr), t, ignore_index=IGNORE)
    (scale * loss).backward()
    return loss.detach(), hr.grad, wr.grad


class TestLinearCrossEntropy:
    TOL = dict(rtol=1e-5, atol=1e-6)

    @pytest.mark.parametrize("chunk_rows", [7, 50, 64])
    def test_matches_torch(self, chunk_rows):
        h, w, t = _head_inputs()
        ref_loss, ref_dh, ref_dw = _torch_head(h, w, t)
        ha = h.clone().requires_grad_(True)
        wa = w.clone().requires_grad_(True)
        loss = linear_cross_entropy(ha, wa, t, chunk_rows=chunk_rows)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        loss.backward()
        torch.testing.assert_close(loss.detach(), ref_loss, **self.TOL)
        torch.testing.assert_close(ha.grad, ref_dh, **self.TOL)
        torch.testing.assert_close(wa.grad, ref_dw, **self.TOL)

    def test_upstream_gradient(self):
        h, w, t = _head_inputs(seed=1)
        _, ref_dh, ref_dw = _torch_head(h, w, t, scale=3.0)
        ha = h.clone().requires_grad_(True)
        wa = w.clone().requires_grad_(True)
        (3 * linear_cross_entropy(ha, wa, t, chunk_rows=7)).backward()
        torch.testing.assert_close(ha.grad, ref_dh, **self.TOL)
        torch.testing.assert_close(wa.grad, ref_dw, **self.TOL)

    def test_h_without_grad(self):
        h, w, t = _head_inputs(seed=2)
        ref_loss, _, ref_dw = _torch_head(h, w, t, h_grad=False)
        wa = w.clone().requires_grad_(True)
        loss = linear_cross_entropy(h, wa, t, chunk_rows=7)
        loss.backward()
        assert h.grad is None
        torch.testing.assert_close(loss.detach(), ref_loss, **self.TOL)
        torch.testing.assert_close(wa.grad, ref_dw, **self.TOL)

    def test_all_ignored_is_zero_not_nan(self):
        h, w, _ = _head_inputs(seed=3)
        t = torch.full((N,), IGNORE)
        ha = h.clone().requires_grad_(True)
        wa = w.clone().requires_grad_(True)
        loss = linear_cross_entropy(ha, wa, t, chunk_rows=7)
        loss.backward()
        assert loss.item() == 0.0
        assert torch.count_nonzero(ha.grad).item() == 0
        assert torch.count_nonzero(wa.grad).item() == 0

    def test_no_grad_and_leading_dims(self):
        h, w, t = _head_inputs(seed=4, ignore_some=False)
        ref_loss, _, _ = _torch_head(h, w, t)
        wa = w.clone().requires_grad_(True)
        with torch.no_grad():
            loss = linear_cross_entropy(h.view(5, 10, D), wa, t.view(5, 10), chunk_rows=7)
        assert not loss.requires_grad
        torch.testing.assert_close(loss, ref_loss, **self.TOL)

    def test_bf16_on_cpu(self):
        h, w, t = _head_inputs(seed=5)
        ref_loss, ref_dh, ref_dw = _torch_head(h, w, t)
        ha = h.bfloat16().requires_grad_(True)
        wa = w.bfloat16().requires_grad_(True)
        loss = linear_cross_entropy(ha, wa, t, chunk_rows=16)
        loss.backward()
        assert loss.dtype == torch.float32
        assert ha.grad.dtype == torch.bfloat16 and wa.grad.dtype == torch.bfloat16
        # bf16 inputs and bf16 GEMM outputs: unit roundoff 2^-8 through a
        # three-GEMM chain
        torch.testing.assert_close(loss, ref_loss, rtol=2e-2, atol=0)
        for got, ref in ((ha.grad, ref_dh), (wa.grad, ref_dw)):
            torch.testing.assert_close(
                got.float(), ref, rtol=3e-2, atol=3e-2 * ref.abs().max().item()
            )

    @pytest.mark.parametrize("chunk_rows", [7, 64])
    def test_bounded_memory(self, chunk_rows):
        h, w, t = _head_inputs(seed=6)
        ha = h.clone().requires_grad_(True)
        wa = w.clone().requires_grad_(True)
        saved = []

        def pack(x):
            saved.append((tuple(x.shape), x.numel() * x.element_size()))
            return x

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda x: x):
            loss = linear_cross_entropy(ha, wa, t, chunk_rows=chunk_rows)
        assert loss.requires_grad
        for shape, _ in saved:
            assert not (len(shape) == 2 and shape[1] == V), (
                f"logits-sized tensor {shape} saved for backward"
            )
        budget = h.numel() * 4 + w.numel() * 4 + 1024
        assert sum(b for _, b in saved) <= budget, saved

    def test_unfused_loop_does_save_logits(self):
        """The same probe on the loop ``Llama.forward_loss`` runs without the
        fused head: it does keep [chunk, V] tensors (what the op removes)."""
        h, w, t = _head_inputs(seed=6)
        ha = h.clone().requires_grad_(True)
        wa = w.clone().requires_grad_(True)
        saved = []

        def pack(x):
            saved.append(tuple(x.shape))
            return x

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda x: x):
            losses = [
                F.cross_entropy(F.linear(ha[i : i + 7], wa), t[i : i + 7], reduction="sum")
                for i in range(0, N, 7)
            ]
            torch.stack(losses).sum()
        assert any(len(s) == 2 and s[1] == V for s in saved)


class TestLlamaSwitch:
    @pytest.fixture(scope="class")
    def model(self):
        torch.manual_seed(0)
        m = Llama(LLAMA_DEBUG, dtype=torch.float32, checkpoint_activations=False)
        return m.train()

    @pytest.fixture(scope="class")
    def batch(self):
        g = torch.Generator().manual_seed(1)
        toks = torch.randint(0, LLAMA_DEBUG.vocab_size, (2, 33), generator=g)
        return toks[:, :-1].contiguous(), toks[:, 1:].contiguous()

    @staticmethod
    def _loss_and_grads(model, loss_fn):
        model.zero_grad(set_to_none=True)
        loss = loss_fn()
        loss.backward()
        return loss.detach().clone(), {
            n: p.grad.detach().clone() for n, p in model.named_parameters()
        }

    @pytest.fixture(scope="class")
    def unfused(self, model, batch):
        x, y = batch
        return self._loss_and_grads(
            model, lambda: model.forward_loss(x, y, chunk_rows=24, fused=False)
        )

    def _check(self, got, unfused):
        loss, grads = got
        ref_loss, ref_grads = unfused
        torch.testing.assert_close(loss, ref_loss, rtol=1e-4, atol=0)
        assert grads.keys() == ref_grads.keys()
        # rtol 1e-4 per element, plus the same 1e-4 taken against the
        # tensor's largest entry: an entry that is a sum cancelling to ~0
        # (abs diff ~1e-8 on tok_embeddings) has no bounded relative error
        # once the two paths sum dlogits in a different order
        for n, g in grads.items():
            torch.testing.assert_close(
                g, ref_grads[n], rtol=1e-4,
                atol=1e-4 * ref_grads[n].abs().max().item(), msg=lambda m: f"{n}: {m}",
            )

    def test_fused_matches_unfused(self, model, batch, unfused):
        x, y = batch
        got = self._loss_and_grads(
            model, lambda: model.forward_loss(x, y, chunk_rows=24, fused=True)
        )
        self._check(got, unfused)

    def test_env_var_switches(self, model, batch, unfused, monkeypatch):
        x, y = batch
        seen = []
        import torchft_amd.models.llama as llama_mod

        real = llama_mod.linear_cross_entropy

        def spy(*a, **k):
            seen.append(1)
            return real(*a, **k)

        monkeypatch.setattr(llama_mod, "linear_cross_entropy", spy)
        monkeypatch.setenv("TORCHFT_AMD_FUSED_CE", "1")
        got = self._loss_and_grads(model, lambda: model.forward_loss(x, y, chunk_rows=24))
        assert seen == [1]
        self._check(got, unfused)
        monkeypatch.setenv("TORCHFT_AMD_FUSED_CE", "0")
        model.forward_loss(x, y, chunk_rows=24)
        monkeypatch.delenv("TORCHFT_AMD_FUSED_CE")
        model.forward_loss(x, y, chunk_rows=24)
        assert seen == [1], "the fused head must stay off by default"

    def test_masking_needs_fused_path(self, model, batch):
        x, y = batch
        with pytest.raises(ValueError):
            model.forward_loss(x, y, fused=False, ignore_index=0)
        with pytest.raises(ValueError):
            model.forward_loss(x, y, fused=False, z_loss=1e-4)

    def test_half_masked_batch(self, model, batch):
        x, y = batch
        y = y.clone()
        y.view(-1)[::2] = IGNORE
        with torch.no_grad():
            loss = model.forward_loss(x, y, chunk_rows=24, fused=True)
            ref = F.cross_entropy(
                model(x).reshape(-1, LLAMA_DEBUG.vocab_size), y.reshape(-1),
                ignore_index=IGNORE,
            )
        torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-6)
