"""The fused QKV split + rotary op and the per-document rotary positions, the
parts that need no GPU: the plain-torch path of ops.qkv_rope against the
slices + rope composition it replaces, DocMask.positions(), and
LlamaConfig.rope_doc_reset in the model."""

import dataclasses

import pytest
import torch

from torchft_amd.models.llama import LLAMA_DEBUG, Llama
from torchft_amd.ops import DocMask, flash_attention, qkv_rope, rope, rope_tables

B, S, HQ, HKV, D = 2, 12, 4, 2, 16
TABLE_ROWS = 20


def _composition(qkv, cos_rows, sin_rows):
    """What Attention.forward did before the fused op: three views of the
    projection and two rope calls. cos_rows / sin_rows: one table per batch
    row, or one for all."""
    nq, nkv = HQ * D, HKV * D
    q = qkv[..., :nq].view(B, S, HQ, D)
    k = qkv[..., nq:nq + nkv].view(B, S, HKV, D)
    v = qkv[..., nq + nkv:].view(B, S, HKV, D)
    if len(cos_rows) == 1:
        return rope(q, cos_rows[0], sin_rows[0]), rope(k, cos_rows[0], sin_rows[0]), v
    q = torch.cat([rope(q[b:b + 1], cos_rows[b], sin_rows[b]) for b in range(B)])
    k = torch.cat([rope(k[b:b + 1], cos_rows[b], sin_rows[b]) for b in range(B)])
    return q, k, v


def _grad_of_qkv(fn, qkv, douts):
    leaf = qkv.detach().clone().requires_grad_(True)
    outs = fn(leaf)
    torch.autograd.backward(outs, douts)
    return [o.detach() for o in outs], leaf.grad


class TestOp:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("with_positions", [False, True], ids=["global", "positions"])
    def test_equals_slices_plus_rope_exactly(self, dtype, with_positions):
        g = torch.Generator().manual_seed(11)
        qkv = torch.randn(B, S, (HQ + 2 * HKV) * D, generator=g).to(dtype)
        douts = [torch.randn(B, S, h, D, generator=g).to(dtype) for h in (HQ, HKV, HKV)]
        cos, sin = rope_tables(TABLE_ROWS, D)
        if with_positions:
            pos = torch.randint(0, TABLE_ROWS, (B, S), generator=g, dtype=torch.int32)
            cos_rows = [cos[pos[b].long()] for b in range(B)]
            sin_rows = [sin[pos[b].long()] for b in range(B)]
        else:
            pos, cos_rows, sin_rows = None, [cos], [sin]

        got, got_grad = _grad_of_qkv(
            lambda t: qkv_rope(t, cos, sin, HQ, HKV, pos), qkv, douts)
        ref, ref_grad = _grad_of_qkv(
            lambda t: _composition(t, cos_rows, sin_rows), qkv, douts)
        for a, b_, h in zip(got, ref, (HQ, HKV, HKV)):
            assert a.shape == (B, S, h, D) and a.dtype == dtype
            assert torch.equal(a, b_)
        assert got_grad.dtype == dtype and torch.equal(got_grad, ref_grad)
        # v is the slice itself
        assert torch.equal(got[2].reshape(B, S, -1), qkv[..., (HQ + HKV) * D:])

    def test_bad_shapes_are_refused(self):
        cos, sin = rope_tables(TABLE_ROWS, D)
        with pytest.raises(ValueError, match="divisible"):
            qkv_rope(torch.zeros(B, S, (HQ + 2 * HKV) * D + 1), cos, sin, HQ, HKV)
        with pytest.raises(ValueError, match="positions"):
            qkv_rope(torch.zeros(B, S, (HQ + 2 * HKV) * D), cos, sin, HQ, HKV,
                     torch.zeros(B, 2 * S, dtype=torch.int32))


def _brute_positions(lengths):
    return [[i for n in row for i in range(n)] for row in lengths]


def _eos_tokens(lengths, eos=7):
    return torch.tensor([[t for n in row for t in [3] * (n - 1) + [eos]]
                         for row in lengths]), eos


class TestDocMaskPositions:
    # one document; a boundary at 1; a boundary at S - 1; a mix
    LAYOUTS = [[[16]], [[1, 15]], [[15, 1]], [[1, 6, 8, 1], [3, 13]]]

    @pytest.mark.parametrize("lengths", LAYOUTS)
    def test_against_a_python_loop(self, lengths):
        n = sum(lengths[0])
        ref = torch.tensor(_brute_positions(lengths), dtype=torch.int32)
        ids = torch.tensor([[d for d, m in enumerate(row) for _ in range(m)]
                            for row in lengths])
        toks, eos = _eos_tokens(lengths)
        for m in (DocMask.from_lengths(lengths, n), DocMask.from_doc_ids(ids),
                  DocMask.from_eos(toks, eos)):
            p = m.positions()
            assert p.dtype == torch.int32 and p.shape == (len(lengths), n)
            assert p.is_contiguous() and p.device == m.doc_start.device
            assert torch.equal(p, ref)

    def test_cached_on_the_instance(self):
        m = DocMask.from_lengths([[5, 11]], 16)
        assert m.positions() is m.positions()
        # the cache is no field: equality and the constructor are as before
        assert dataclasses.fields(m)[0].name == "doc_start" and len(dataclasses.fields(m)) == 2
        with pytest.raises(AttributeError):
            m.doc_start = m.doc_end


class TestModel:
    LA, LB = 1984, 64

    def _model(self, reset, **kw):
        cfg = dataclasses.replace(LLAMA_DEBUG, max_seq_len=self.LA + self.LB,
                                  rope_doc_reset=reset)
        torch.manual_seed(5)
        return Llama(cfg, dtype=torch.float32, checkpoint_activations=False, **kw).eval()

    def test_document_independence(self):
        """A row packs documents A (1984 tokens) and B (64); B is also run
        alone. With rope_doc_reset B's hidden states in the packed row are
        those of B alone; with global positions they are not.

        Measured on the CPU in fp32 (LLAMA_DEBUG sizes, max|hidden| = 4.26):
        e_reset = 0.0 exactly (the same table rows and the same arithmetic
        reach B either way), e_global = 3.6e-6. Rotary attention scores depend
        on the distance between query and key only, so in exact arithmetic
        global positions would give B the same states too; what B sees at
        offset 1984 is the fp32 rounding of the angles there (1984 * 2^-24 =
        1.2e-4 rad at the highest frequency), which the reset removes. At an
        offset of 448 e_global is 2.1e-6."""
        S = self.LA + self.LB
        toks = torch.randint(0, LLAMA_DEBUG.vocab_size, (1, S),
                             generator=torch.Generator().manual_seed(6))
        m = DocMask.from_lengths([[self.LA, self.LB]], S)
        err = {}
        for reset in (True, False):
            model = self._model(reset)
            with torch.no_grad():
                packed = model.forward_hidden(toks, doc_mask=m)[:, self.LA:]
                alone = model.forward_hidden(toks[:, self.LA:])
            err[reset] = (packed - alone).abs().max().item()
            scale = alone.abs().max().item()
        e_reset, e_global = err[True], err[False]
        print(f"e_reset {e_reset:.3e}  e_global {e_global:.3e}  max|hidden| {scale:.3f}")
        assert e_reset * 1000 <= e_global
        assert e_global > 0
        assert e_reset <= 1e-4 * scale

    def test_default_config_is_the_parents_path(self):
        """rope_doc_reset=False, with and without a mask: exactly the hidden
        states of three views + two rope calls, inlined here."""
        assert LLAMA_DEBUG.rope_doc_reset is False
        model = self._model(False)
        cfg = model.cfg
        toks = torch.randint(0, cfg.vocab_size, (2, 128),
                             generator=torch.Generator().manual_seed(8))
        m = DocMask.from_lengths([[40, 88], [128]], 128)

        def parent_hidden(doc_mask):
            x = model.tok_embeddings(toks)
            Bt, St, hd = 2, 128, cfg.head_dim
            nq, nkv = cfg.n_heads * hd, cfg.n_kv_heads * hd
            for layer in model.layers:
                qkv = layer.attn.wqkv(layer.attn_norm(x))
                q = qkv[..., :nq].view(Bt, St, cfg.n_heads, hd)
                k = qkv[..., nq:nq + nkv].view(Bt, St, cfg.n_kv_heads, hd)
                v = qkv[..., nq + nkv:].view(Bt, St, cfg.n_kv_heads, hd)
                q, k = rope(q, model.rope_cos, model.rope_sin), rope(k, model.rope_cos, model.rope_sin)
                out = flash_attention(*(t.transpose(1, 2) for t in (q, k, v)),
                                      causal=True, doc_mask=doc_mask)
                x = x + layer.attn.wo(out.transpose(1, 2).reshape(Bt, St, -1))
                x = x + layer.mlp(layer.mlp_norm(x))
            return model.norm(x)

        with torch.no_grad():
            for doc_mask in (None, m):
                assert torch.equal(model.forward_hidden(toks, doc_mask=doc_mask),
                                   parent_hidden(doc_mask))

    def test_reset_without_a_mask_changes_nothing(self):
        toks = torch.randint(0, LLAMA_DEBUG.vocab_size, (1, 64),
                             generator=torch.Generator().manual_seed(9))
        with torch.no_grad():
            assert torch.equal(self._model(True).forward_hidden(toks),
                               self._model(False).forward_hidden(toks))

    def test_reset_trains_through_checkpointing(self):
        cfg = dataclasses.replace(LLAMA_DEBUG, rope_doc_reset=True)
        torch.manual_seed(7)
        model = Llama(cfg, dtype=torch.float32, checkpoint_activations=True).train()
        toks = torch.randint(0, cfg.vocab_size, (2, 129))
        m = DocMask.from_lengths([[40, 88], [128]], 128)
        loss = model.forward_loss(toks[:, :-1], toks[:, 1:], doc_mask=m)
        loss.backward()
        assert torch.isfinite(loss)
        assert torch.isfinite(model.layers[0].attn.wqkv.weight.grad).all()
        model.checkpoint_activations = False
        torch.testing.assert_close(
            model.forward_loss(toks[:, :-1], toks[:, 1:], doc_mask=m), loss,
            rtol=1e-6, atol=1e-6)

    def test_head_dim_must_be_a_multiple_of_16(self):
        cfg = dataclasses.replace(LLAMA_DEBUG, dim=96, n_heads=4, n_kv_heads=2,
                                  rope_doc_reset=True)
        assert cfg.head_dim == 24
        with pytest.raises(ValueError, match="head_dim % 16"):
            Llama(cfg, dtype=torch.float32)
        # without the reset the same sizes are fine
        Llama(dataclasses.replace(cfg, rope_doc_reset=False), dtype=torch.float32)
