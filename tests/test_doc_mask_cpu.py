"""Document masks for packed sequences, the parts that need no GPU: the
DocMask constructors, the dense-mask fallback of flash_attention, its argument
checks and the doc_mask keyword of the Llama model."""

import pytest
import torch
import torch.nn.functional as F

from torchft_amd.models.llama import LLAMA_DEBUG, CPPlan, Llama
from torchft_amd.ops import DocMask, flash_attention

LAYOUTS = [[1, 31, 32, 33, 63, 96], [256]]
S = 256


def _brute(lengths):
    """doc_start / doc_end of one row by a plain Python loop."""
    ds, de = [], []
    at = 0
    for n in lengths:
        for _ in range(n):
            ds.append(at)
            de.append(at + n)
        at += n
    return ds, de


def _ids(lengths):
    return torch.tensor([[d for d, n in enumerate(row) for _ in range(n)]
                         for row in lengths])


def _eos_tokens(lengths, eos=7):
    """Tokens whose EOS positions end the documents of `lengths`; the last
    document of a row ends with the row, with or without an EOS."""
    rows = []
    for r, row in enumerate(lengths):
        toks = []
        for n in row:
            toks += [3] * (n - 1) + [eos]
        if r % 2 == 0:
            toks[-1] = 3  # an unterminated last document
        rows.append(toks)
    return torch.tensor(rows), eos


class TestConstructors:
    def test_agree_with_each_other_and_brute_force(self):
        m_len = DocMask.from_lengths(LAYOUTS, S)
        m_ids = DocMask.from_doc_ids(_ids(LAYOUTS))
        toks, eos = _eos_tokens(LAYOUTS)
        m_eos = DocMask.from_eos(toks, eos)
        ref_s = torch.tensor([_brute(row)[0] for row in LAYOUTS], dtype=torch.int32)
        ref_e = torch.tensor([_brute(row)[1] for row in LAYOUTS], dtype=torch.int32)
        for m in (m_len, m_ids, m_eos):
            assert m.doc_start.dtype == torch.int32 and m.doc_end.dtype == torch.int32
            assert m.doc_start.shape == (2, S) and m.doc_end.shape == (2, S)
            assert m.doc_start.is_contiguous() and m.doc_end.is_contiguous()
            assert torch.equal(m.doc_start, ref_s)
            assert torch.equal(m.doc_end, ref_e)

    def test_ids_need_not_be_sorted_or_dense(self):
        # a new document wherever the id changes, whatever the ids are
        ids = torch.tensor([[9, 9, 2, 2, 2, 9, 5, 5]])
        m = DocMask.from_doc_ids(ids)
        assert m.doc_start.tolist() == [[0, 0, 2, 2, 2, 5, 6, 6]]
        assert m.doc_end.tolist() == [[2, 2, 5, 5, 5, 6, 8, 8]]

    def test_monotone_and_consistent(self):
        g = torch.Generator().manual_seed(0)
        ids = torch.randint(0, 3, (4, 97), generator=g)
        m = DocMask.from_doc_ids(ids)
        pos = torch.arange(97)
        assert (m.doc_start[:, 1:] >= m.doc_start[:, :-1]).all()
        assert (m.doc_end[:, 1:] >= m.doc_end[:, :-1]).all()
        assert (m.doc_start <= pos).all() and (m.doc_end > pos).all()
        # the end of the document that starts at doc_start[i] is doc_end[i]
        assert torch.equal(torch.gather(m.doc_end, 1, m.doc_start.long()), m.doc_end)

    def test_lengths_must_sum_to_s(self):
        with pytest.raises(ValueError, match="sum to 256"):
            DocMask.from_lengths([[100, 100]], S)
        with pytest.raises(ValueError, match="positive"):
            DocMask.from_lengths([[0, 256]], S)

    def test_immutable(self):
        m = DocMask.from_lengths([[256]], S)
        with pytest.raises(AttributeError):
            m.doc_start = m.doc_end

    def test_dense_is_both_rules(self):
        m = DocMask.from_lengths(LAYOUTS, S)
        d = m.dense()
        assert d.shape == (2, 1, S, S) and d.dtype == torch.bool
        pos = torch.arange(S)
        i, j = pos[:, None], pos[None, :]
        by_start = (j <= i) & (j >= m.doc_start[:, :, None])
        by_end = (i < m.doc_end[:, None, :]) & (j <= i)
        assert torch.equal(d[:, 0], by_start)
        assert torch.equal(d[:, 0], by_end)


def _block_diagonal(q, k, v, lengths):
    """Each document on its own through causal SDPA."""
    out = torch.empty_like(q)
    for b, row in enumerate(lengths):
        at = 0
        for n in row:
            sl = slice(at, at + n)
            out[b, :, sl] = F.scaled_dot_product_attention(
                q[b : b + 1, :, sl], k[b : b + 1, :, sl], v[b : b + 1, :, sl],
                is_causal=True, enable_gqa=q.shape[1] != k.shape[1],
            )[0]
            at += n
    return out


class TestFallback:
    @pytest.mark.parametrize("Hq,Hkv", [(2, 2), (4, 2)])
    def test_cpu_fp32_equals_per_document_attention(self, Hq, Hkv):
        torch.manual_seed(3)
        B, D = 2, 32

        def mk(H):
            return torch.randn(B, H, S, D, requires_grad=True)

        q, k, v = mk(Hq), mk(Hkv), mk(Hkv)
        g = torch.randn(B, Hq, S, D)
        m = DocMask.from_lengths(LAYOUTS, S)
        out = flash_attention(q, k, v, causal=True, doc_mask=m)
        out.backward(g)
        q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        ref = _block_diagonal(q2, k2, v2, LAYOUTS)
        ref.backward(g)
        torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(q.grad, q2.grad, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(k.grad, k2.grad, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(v.grad, v2.grad, rtol=1e-5, atol=1e-5)

    def test_no_mask_is_unchanged(self):
        torch.manual_seed(4)
        q, k, v = (torch.randn(1, 2, 64, 32) for _ in range(3))
        ref = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        assert torch.equal(flash_attention(q, k, v, causal=True), ref)
        assert torch.equal(flash_attention(q, k, v, causal=True, doc_mask=None), ref)

    def test_non_causal_mask_is_refused(self):
        q, k, v = (torch.randn(1, 2, S, 32) for _ in range(3))
        m = DocMask.from_lengths([[256]], S)
        with pytest.raises(ValueError, match="causal"):
            flash_attention(q, k, v, causal=False, doc_mask=m)


class TestModel:
    LENGTHS = [[40, 88], [128]]
    SEQ = 128

    def _model(self, **kw):
        torch.manual_seed(5)
        return Llama(LLAMA_DEBUG, dtype=torch.float32, checkpoint_activations=False,
                     **kw).eval()

    def test_mask_changes_logits_and_isolates_documents(self):
        """Rotary positions stay global, but RoPE scores depend only on the
        distance between query and key, so a document at offset p gives the
        logits it gives alone at offset 0 up to fp32 rounding of the
        rotations (eps 6e-8 times a few hundred operations: 1e-4 is ample)."""
        model = self._model()
        toks = torch.randint(0, LLAMA_DEBUG.vocab_size, (2, self.SEQ),
                             generator=torch.Generator().manual_seed(6))
        m = DocMask.from_lengths(self.LENGTHS, self.SEQ)
        with torch.no_grad():
            plain = model(toks)
            masked = model(toks, doc_mask=m)
            hidden = model.forward_hidden(toks, doc_mask=m)
            assert torch.equal(model.output(hidden), masked)
            # row 1 is one document: the mask changes nothing there
            torch.testing.assert_close(masked[1], plain[1], rtol=1e-4, atol=1e-4)
            # row 0: the first document is unchanged, the second one is not
            torch.testing.assert_close(masked[0, :40], plain[0, :40], rtol=1e-4, atol=1e-4)
            assert (masked[0, 40:] - plain[0, 40:]).abs().max() > 1e-2
            for b, row in enumerate(self.LENGTHS):
                at = 0
                for n in row:
                    alone = model(toks[b : b + 1, at : at + n])
                    torch.testing.assert_close(masked[b : b + 1, at : at + n], alone,
                                               rtol=1e-4, atol=1e-4)
                    at += n

    def test_forward_loss_and_checkpointing_take_the_mask(self):
        torch.manual_seed(7)
        model = Llama(LLAMA_DEBUG, dtype=torch.float32, checkpoint_activations=True)
        model.train()
        toks = torch.randint(0, LLAMA_DEBUG.vocab_size, (2, self.SEQ + 1))
        m = DocMask.from_lengths(self.LENGTHS, self.SEQ)
        loss_m = model.forward_loss(toks[:, :-1], toks[:, 1:], doc_mask=m)
        loss_m.backward()
        grad_m = model.layers[0].attn.wqkv.weight.grad.clone()
        model.zero_grad()
        loss_p = model.forward_loss(toks[:, :-1], toks[:, 1:])
        loss_p.backward()
        assert torch.isfinite(loss_m) and loss_m.item() != loss_p.item()
        assert not torch.equal(grad_m, model.layers[0].attn.wqkv.weight.grad)
        # checkpointed and plain forward agree
        model.checkpoint_activations = False
        torch.testing.assert_close(
            model.forward_loss(toks[:, :-1], toks[:, 1:], doc_mask=m), loss_m,
            rtol=1e-6, atol=1e-6)

    def test_context_parallel_refuses_the_mask(self):
        model = self._model(cp=CPPlan(pg=None, rank=0, world=2))
        toks = torch.zeros(1, 64, dtype=torch.long)
        m = DocMask.from_lengths([[64]], 64)
        with pytest.raises(NotImplementedError, match="doc_mask"):
            model(toks, doc_mask=m)
        with pytest.raises(NotImplementedError, match="doc_mask"):
            model.forward_loss(toks, toks, doc_mask=m)
