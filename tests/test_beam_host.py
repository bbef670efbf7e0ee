"""The host model of the decode bookkeeping (tests/beam_ref.py) pinned to the CPU oracle: driven
step by step on a toy ``forward``, beam_step reproduces oracle.model.beam_search's best-beam
captions for every beam size, greedy_step reproduces oracle.model.greedy, and beam 1 == greedy.
No GPU: the device tests compare the kernels with this model, so it has to be right first."""
import numpy as np
import pytest
import torch

from oracle import model as orc
from tests.beam_ref import (beam_init, beam_step, best_captions, copy_state, greedy_init,
                            greedy_step)

V, B, T, BOS = 50, 3, 12, 1
EOS_EARLY, EOS_SOME = 2, 7


def _table():
    """logits[r, t, :] = table[caption[r, t], t]: half-integer values (many equal logits within a
    row), two equal best words at step 0 whose rows at step 1 are identical (equal totals across
    two parents), a boost of EOS_SOME so beams finish at different steps, and EOS_EARLY the
    overwhelming choice of every row at step 3 (that choice of EOS ends the search there)."""
    g = torch.Generator().manual_seed(5)
    tab = torch.round(torch.randn(V, T, V, generator=g) * 4) / 2
    tab[:, 0, 5] = tab[:, 0, 9] = 9.0
    tab[9, 1] = tab[5, 1]
    tab[:, 1, 11] = tab[:, 1, 12] = tab[:, 1, 13] = 8.0
    tab[::2, 2, EOS_SOME] += 5.0
    tab[1::3, 6, EOS_SOME] += 5.0
    tab[:, 3, EOS_EARLY] = 40.0
    return tab


TABLE = _table()


def forward(caption, mask):
    return TABLE[caption, torch.arange(caption.shape[1])[None, :]]


def _candidates(hist, i, K):
    """The oracle's per-row candidates of step i (fp32 log-sum-exp, stable descending sort)."""
    logits = TABLE[torch.from_numpy(hist[:, i]), i].float()
    lse = torch.logsumexp(logits, -1, keepdim=True)
    vals, idx = torch.sort(logits, dim=-1, descending=True, stable=True)
    return idx[:, :K].numpy(), (vals[:, :K] - lse).numpy()


def _drive_beam(K, eos):
    st = beam_init(B, K, T, BOS)
    for i in range(T - 1):
        tok, lp = _candidates(st["hist"], i, K)
        before = copy_state(st)
        st = beam_step(st, tok, lp, i, eos)
        if before["done"] >= 0:                       # nothing moves once the search has ended
            for k, v in before.items():
                assert np.array_equal(v, st[k]), k
    return st


@pytest.mark.parametrize("eos", [EOS_EARLY, EOS_SOME])
@pytest.mark.parametrize("K", range(1, 9))
def test_beam_step_matches_oracle_beam_search(K, eos):
    st = _drive_beam(K, eos)
    ref = orc.beam_search(forward, B, T, K, BOS, eos)
    assert np.array_equal(best_captions(st, B, K), ref.numpy()), (K, eos)
    if eos == EOS_EARLY:
        assert st["done"] == 3                        # the planted early end
        assert not ref[:, 5:].any()
    else:
        fin = st["finished"].reshape(B, K)
        # finished beams live to the last step beside open ones
        assert st["done"] == -1 and (K == 1 or fin.any()) and not fin.all()
    # ancestry: every entry names a row of the same image
    rows = np.arange(B * K)[:, None] // K
    assert np.array_equal(st["anc"] // K, np.broadcast_to(rows, st["anc"].shape))


def _drive_greedy(eos, write_all=False):
    st = greedy_init(B, T, BOS)
    for i in range(T - 1):
        pred = TABLE[torch.from_numpy(st["tok"]), i].numpy().argmax(-1)   # first index on ties
        st = greedy_step(st, pred, i, eos, write_all)
    return st


@pytest.mark.parametrize("eos", [EOS_EARLY, EOS_SOME, -1])
def test_greedy_step_matches_oracle_and_beam1(eos):
    g = _drive_greedy(eos)
    ref = orc.greedy(forward, B, T, BOS, eos)
    assert np.array_equal(g["caption"], ref.numpy())
    b1 = _drive_beam(1, eos)
    assert np.array_equal(best_captions(b1, B, 1), g["caption"])
    assert b1["done"] == g["done"]
    assert np.array_equal(b1["finished"], g["finished"])


def test_greedy_step_write_all_keeps_first_done():
    """write_all: every column is written and done stays at the first all-finished step."""
    g, w = _drive_greedy(EOS_EARLY), _drive_greedy(EOS_EARLY, write_all=True)
    assert g["done"] == w["done"] == 3
    assert np.array_equal(g["caption"][:, :4], w["caption"][:, :4])
    assert not g["caption"][:, 4:].any() and (w["caption"][:, 4] == EOS_EARLY).all()
    assert np.array_equal(g["tok"], w["tok"])
