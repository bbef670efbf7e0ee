"""The greedy decode bookkeeping kernels (csrc/loss.hip: retr_greedy_update, retr_greedy_select,
retr_greedy_select2 with both write_all values) against the host model of the decode contract
(tests/beam_ref.py greedy_step, pinned to oracle.model.greedy by tests/test_beam_host.py) over
eight consecutive steps: planted argmax positions and exact ties (first index wins), rows that
reach EOS at different steps, all of them by step 5, and the steps after ``done`` is set.
Everything is integer state, so every comparison is exact."""
import numpy as np
import pytest
import torch

from retr_amd import _lib, ops
from retr_amd._lib import call, ptr
from tests.beam_ref import greedy_init, greedy_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, STEPS, EOS, BOS, ALL_DONE, UNWRITTEN = 12, 8, 102, 101, 5, -7


def _plan(B, V, seed):
    """Per step: the bf16 logits [B, ld] and their first-index argmax.  Row b's best word is
    planted (40.0) at a random position, in every third row twice (an exact tie; the reference
    argmax takes the first), and is EOS at step fs[b] in 0 .. 5, the last row's at step 5: rows
    finish at different steps and all are finished at step 5.  Pad columns hold +1e30."""
    ld = (V + 7) // 8 * 8
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    fs = (np.arange(B) * 7) % (ALL_DONE + 1)
    fs[-1] = ALL_DONE
    rows = np.arange(B)
    steps = []
    for i in range(STEPS):
        x = torch.randn(B, ld, generator=g) * 3
        pos = rng.integers(0, V, B)
        pos[pos == EOS] = EOS + 1
        pos[fs == i] = EOS
        x[rows, pos] = 40.0
        tie = rows[(rows % 3 == 1) & (fs != i)]
        other = rng.integers(0, V, tie.shape[0])
        other[other == EOS] = EOS + 1
        x[tie, other] = 40.0
        x[:, V:] = 1e30
        xb = x.bfloat16()
        pred = xb[:, :V].float().numpy().argmax(-1)              # numpy: the first maximum
        want = pos.copy()
        want[tie] = np.minimum(pos[tie], other)
        assert np.array_equal(pred, want)                        # the plan is what was planted
        steps.append((xb, pred.astype(np.int64)))
    return ld, steps


def _dev_state(st):
    return dict(caption=torch.from_numpy(st["caption"]).to(DEV),
                finished=torch.from_numpy(st["finished"]).to(DEV),
                tok=torch.from_numpy(st["tok"]).to(DEV),
                done=torch.tensor([st["done"]], dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("fn,write_all", [("update", 0), ("select", 0), ("select2", 0),
                                          ("select2", 1)])
@pytest.mark.parametrize("V,B", [(8200, 1), (8200, 3), (8200, 64), (8200, 300), (1003, 1),
                                 (1003, 3), (1003, 64), (1003, 300), (1003, 1025)])
def test_greedy_state_matches_host_model(fn, write_all, V, B):
    """V = 8200 takes the fused argmax_part + greedy_select path, V = 1003 (and B = 1025 > 1024)
    the retr_argmax_rows + greedy_update fallback; B > 256 makes the bookkeeping loops iterate.
    After every step pred, caption, finished, done and tok equal the model.  write_all = 0: the
    columns from done + 1 on are never written while tok still follows pred; write_all = 1: every
    column is written and done keeps the first all-finished step."""
    ld, steps = _plan(B, V, seed=V + B)
    m = greedy_init(B, T, BOS, fill=UNWRITTEN)
    d = _dev_state(m)
    pred = torch.full((B,), -1, dtype=torch.long, device=DEV)
    ws = torch.empty(_lib.load().retr_argmax_workspace(B), dtype=torch.uint8, device=DEV)
    st = ops._st()
    for i, (xb, ref_pred) in enumerate(steps):
        xd = xb.to(DEV)
        tail = (ptr(d["caption"]), ptr(d["finished"]), ptr(d["done"]), ptr(d["tok"]))
        if fn == "update":
            pred.copy_(torch.from_numpy(ref_pred))
            call("retr_greedy_update", ptr(pred), B, T, i, EOS, *tail, st)
        elif fn == "select":
            call("retr_greedy_select", 1, ptr(xd), ld, B, V, ptr(ws), T, i, EOS, ptr(pred),
                 *tail, st)
        else:
            call("retr_greedy_select2", 1, ptr(xd), ld, B, V, ptr(ws), T, i, EOS, ptr(pred),
                 *tail, write_all, st)
        torch.cuda.synchronize()
        m = greedy_step(m, ref_pred, i, EOS, bool(write_all))
        assert torch.equal(pred.cpu(), torch.from_numpy(ref_pred)), i
        assert torch.equal(d["caption"].cpu(), torch.from_numpy(m["caption"])), i
        assert torch.equal(d["finished"].cpu(), torch.from_numpy(m["finished"])), i
        assert torch.equal(d["tok"].cpu(), torch.from_numpy(m["tok"])), i
        assert int(d["done"][0]) == m["done"] == (ALL_DONE if i >= ALL_DONE else -1), i
    cap = d["caption"].cpu().numpy()
    assert (cap[:, 1:ALL_DONE + 1] != UNWRITTEN).all()
    if write_all:
        assert (cap[:, ALL_DONE + 1:STEPS + 1] != UNWRITTEN).all()
        assert np.array_equal(cap[:, STEPS], steps[-1][1])
    else:
        assert (cap[:, ALL_DONE + 1:] == UNWRITTEN).all()
    assert (cap[:, STEPS + 1:] == UNWRITTEN).all()
    assert np.array_equal(d["tok"].cpu().numpy(), steps[-1][1])
