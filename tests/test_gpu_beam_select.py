"""retr_beam_select and retr_topk_rows (csrc/beam.hip) against host references.

retr_beam_select is driven step by step beside the numpy model of one beam step
(tests/beam_ref.py, pinned to the CPU oracle by tests/test_beam_host.py) on host-made candidate
streams with planted ties, EOS and early ends: every state tensor is compared exactly after
every step (integer state, and scores that are one fp32 add per step).  retr_topk_rows is
compared with a stable sort and a float64 log-softmax for every K of both kernels and both
dtypes, on poisoned pad columns, -inf logits and large magnitudes."""
import numpy as np
import pytest
import torch

from retr_amd import ops
from retr_amd._lib import call, ptr
from tests.beam_ref import beam_candidates, beam_init, beam_step, copy_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOS, EOS, NTOK = 101, 999, 997          # candidate tokens are drawn from [0, NTOK), EOS planted


# ---------------------------------------------------------------- retr_beam_select
def _to_dev(st):
    d = {k: torch.from_numpy(v).to(DEV) for k, v in st.items() if k != "done"}
    d["done"] = torch.tensor([st["done"]], dtype=torch.int32, device=DEV)
    return d


def _select(d, cand_tok, cand_lp, B, K, i, T, eos=EOS):
    ct = torch.from_numpy(np.ascontiguousarray(cand_tok, dtype=np.int32)).to(DEV)
    cl = torch.from_numpy(np.ascontiguousarray(cand_lp, dtype=np.float32)).to(DEV)
    call("retr_beam_select", ptr(ct), ptr(cl), B, K, i, T, eos, ptr(d["scores"]),
         ptr(d["finished"]), ptr(d["hist"]), ptr(d["anc"]), ptr(d["tok"]), ptr(d["item_done"]),
         ptr(d["done"]), ops._st())
    torch.cuda.synchronize()


def _host(d):
    h = {k: v.cpu() for k, v in d.items()}
    h["done"] = int(h["done"][0])
    return h


def _assert_state(h, m, ctx, scores_exact=True):
    """Device state h (host copies) == model state m, bit for bit."""
    for k in ("finished", "hist", "anc", "tok", "item_done"):
        assert torch.equal(h[k], torch.from_numpy(m[k])), (k, ctx)
    assert h["done"] == m["done"], ("done", ctx, h["done"], m["done"])
    if scores_exact:
        assert torch.equal(h["scores"].view(torch.int32),
                           torch.from_numpy(m["scores"]).view(torch.int32)), ("scores", ctx)


def _make_cands(rng, B, K, i, finish_all=False):
    """Candidates of step i: cand_tok distinct within a row, cand_lp negative and non-increasing.
    Rows of even images, and two steps out of three of odd images, carry quarter-integer values
    (every total is then exact in fp32, so equal totals across parents and equal lp within a row
    are frequent); the other rows carry arbitrary fp32 values (the add rounds).  EOS is sprinkled
    over the images between the first and the last; image 0 finishes entirely at step 2
    (``finish_all``: every image does, at this step): EOS best in every row, the rest far below."""
    R = B * K
    start, stride = rng.integers(0, NTOK, R), rng.integers(1, NTOK, R)
    tok = ((start[:, None] + np.arange(K)[None, :] * stride[:, None]) % NTOK).astype(np.int32)
    inc = rng.integers(0, 3, (R, K))
    inc[:, 0] = rng.integers(1, 4, R)
    lp = (-np.cumsum(inc, 1) / 4.0).astype(np.float32)
    flt = -np.cumsum(rng.random((R, K), dtype=np.float32) + np.float32(0.01), 1,
                     dtype=np.float32)
    img = np.arange(R) // K
    use_flt = (img % 2 == 1) & (i % 3 == 2)
    lp[use_flt] = flt[use_flt]
    if i >= 1:
        plant = (rng.random(R) < 0.08) & (img > 0) & (img < B - 1)
        rank = rng.integers(0, K, R)
        tok[plant, rank[plant]] = EOS
    ends = np.ones(R, bool) if finish_all else ((img == 0) & (i == 2))
    if ends.any():
        tok[ends, 0] = EOS
        lp[ends, 0] = -0.25
        lp[ends, 1:] = (-1000.0 - np.arange(K - 1)).astype(np.float32)
    return tok, lp


def _tie_counts(st, tok, lp, B, K, i):
    """How many images have, among their K + 1 best candidates, two equal totals from different
    parents / from the same parent (the orders the tie rule decides)."""
    cross = within = 0
    for b in range(B):
        c = beam_candidates(st["scores"], st["finished"], tok, lp, b * K, K, i)
        top = sorted(range(len(c)), key=lambda q: (-float(c[q][0]), q))[:K + 1]
        for x, y in zip(top, top[1:]):
            if c[x][0] == c[y][0]:
                cross += c[x][1] != c[y][1]
                within += c[x][1] == c[y][1]
    return cross, within


def _drive(B, K, T, seed, finish_all_at=None, extra_calls=0, count_ties=False):
    """Kernel and model side by side over the steps; returns (model state, tie counts)."""
    rng = np.random.default_rng(seed)
    m = beam_init(B, K, T, BOS)
    d = _to_dev(m)
    R = B * K
    rows = np.arange(R)[:, None]
    fed = np.full((R, T), -1, np.int64)           # fed[r][t]: the token row r consumed at t
    cross = within = 0
    last = T - 2 if finish_all_at is None else finish_all_at + extra_calls
    for i in range(last + 1):
        tok, lp = _make_cands(rng, B, K, i, finish_all=(i == finish_all_at))
        live = m["done"] < 0
        if count_ties and live:
            c, w = _tie_counts(m, tok, lp, B, K, i)
            cross, within = cross + c, within + w
        fed[:, i] = d["tok"].cpu().numpy()
        before = _host(d)
        _select(d, tok, lp, B, K, i, T)
        m = beam_step(m, tok, lp, i, EOS)
        h = _host(d)
        _assert_state(h, m, (B, K, T, i))
        if not live:                              # early return: every tensor bit-identical
            for k in before:
                same = before[k] == h[k] if k == "done" else torch.equal(
                    before[k].view(torch.uint8), h[k].view(torch.uint8))
                assert same, (k, i)
            continue
        # what the decode attention relies on: anc[r][t] names the row of the same image whose
        # cache holds position t of beam r, i.e. the row that consumed hist[r][t] at step t
        a, hist = h["anc"].numpy(), h["hist"].numpy()
        assert np.array_equal(a // K, np.broadcast_to(rows // K, a.shape)), i
        t = np.arange(i + 1)
        assert np.array_equal(fed[a[:, :i + 1], t[None, :]], hist[:, :i + 1]), i
    return m, (cross, within)


@pytest.mark.parametrize("B,T", [(1, 4), (3, 20), (64, 128)])
@pytest.mark.parametrize("K", range(1, 9))
def test_beam_select_matches_host_model(K, B, T):
    """Every step i = 0 .. T-2 of a search with planted ties (lower parent, then lower rank),
    EOS at scattered steps (finished beams live through the later steps), image 0 finishing at
    step 2 while the others go on: scores (bitwise), finished, hist, anc, tok, item_done and done
    equal the host model after every step, and the ancestry stays consistent with what each
    cache row was fed."""
    m, (cross, within) = _drive(B, K, T, seed=1000 * K + T, count_ties=(B, T) == (3, 20))
    if T > 4:
        assert m["item_done"][0] == 1 and m["finished"][:K].all()
    if B > 1:
        assert m["done"] == -1 and not m["finished"][-K:].any()   # the last image never ends
    else:
        assert m["done"] == 2                                     # the only image ended at T-2
    if (B, T) == (3, 20) and K > 1:
        assert cross > 0 and within > 0, (cross, within)          # the planted ties were decisive


@pytest.mark.parametrize("K", range(1, 9))
def test_beam_select_stops_after_done(K):
    """All images finish at step i0 = 9 < T-2: done = i0, and two further calls change nothing."""
    m, _ = _drive(3, K, 20, seed=77 + K, finish_all_at=9, extra_calls=2)
    assert m["done"] == 9 and m["finished"].all() and m["item_done"].all()


def _random_state(rng, B, K, T, i):
    """A mid-search state at step i: arbitrary history, some beams finished, descending scores
    per image, and arbitrary rows of the same image in EVERY ancestry column.  In a search driven
    from the start anc[r][t] == r for t >= i, which would hide a missing anc[s][i] = parent
    write behind the earlier steps' anc[s][t > i] = s; here both writes show."""
    R = B * K
    st = beam_init(B, K, T, BOS)
    st["hist"][:, 1:i + 1] = rng.integers(0, NTOK, (R, i))
    st["hist"][:, i + 1:] = -3                      # columns the step must carry over untouched
    st["anc"][:] = (np.arange(R)[:, None] // K * K + rng.integers(0, K, (R, T))).astype(np.int32)
    st["scores"] = (-np.sort(rng.random((B, K), dtype=np.float32) * 40, axis=1)).reshape(R)
    st["finished"] = (rng.random(R) < 0.3).astype(np.uint8)
    st["tok"] = st["hist"][:, i].copy()
    return st


@pytest.mark.parametrize("K", range(1, 9))
def test_beam_select_step_from_arbitrary_state(K):
    """One step at i = 1, 4 and T-2 from states no search from the start reaches (see
    _random_state): the survivors' rows are the parents' rows with exactly column i + 1 of hist,
    column i of anc (the parent's row) and the columns after i of anc (the own row) rewritten."""
    B, T = 5, 9
    rng = np.random.default_rng(40 + K)
    for i in (1, 4, T - 2):
        m = _random_state(rng, B, K, T, i)
        d = _to_dev(m)
        tok, lp = _make_cands(rng, B, K, i)
        _select(d, tok, lp, B, K, i, T)
        _assert_state(_host(d), beam_step(m, tok, lp, i, EOS), (K, i))


def test_beam_select_largest_rows():
    """K = 8, T = 682: the largest K*T whose staged rows fit the 64 KiB LDS limit is accepted and
    one step from a mid-search state matches the model."""
    B, K, T, i = 2, 8, 682, 340
    rng = np.random.default_rng(682)
    m = _random_state(rng, B, K, T, i)
    d = _to_dev(m)
    tok, lp = _make_cands(rng, B, K, i)
    _select(d, tok, lp, B, K, i, T)
    _assert_state(_host(d), beam_step(m, tok, lp, i, EOS), (B, K, T, i))


@pytest.mark.parametrize("K,i,T", [(0, 1, 16), (9, 1, 16), (3, 15, 16), (8, 1, 683)])
def test_beam_select_rejects_bad_arguments(K, i, T):
    """K outside [1, 8], i + 1 == T and K*T over the LDS limit fail on the host (RuntimeError
    from call) before anything is launched: the state is untouched.  The buffers are sized for
    the dimensions passed, so nothing could be read or written out of bounds either way."""
    B, Ka = 2, max(K, 1)
    rng = np.random.default_rng(K * 1000 + T)
    m = _random_state(rng, B, Ka, T, min(i, T - 2))
    d = _to_dev(m)
    tok, lp = _make_cands(rng, B, Ka, 1)
    with pytest.raises(RuntimeError, match="beam_select"):
        _select(d, tok, lp, B, K, i, T)
    torch.cuda.synchronize()
    _assert_state(_host(d), m, (K, i, T))


def _f64_candidates(x, V, K):
    """Per row of x [R, ld]: the K best words by a stable descending sort (value, then index) and
    their float64 log-softmax over the first V columns."""
    xf = x[:, :V].float().cpu()
    _, order = torch.sort(xf, dim=-1, descending=True, stable=True)
    lp = torch.log_softmax(xf.double(), -1)
    idx = order[:, :K]
    return idx.numpy().astype(np.int32), lp.gather(1, idx).numpy()


def test_topk_feeds_beam_select_bf16():
    """retr_topk_rows -> retr_beam_select at the cfg5 vocabulary (B 4, K 5, V 30522, bf16) over 6
    steps against the model fed float64 candidates: the token state (hist, anc, tok, finished,
    item_done, done) is identical; the scores agree to the fp32 log-softmax tolerance."""
    B, K, V, T, steps, eos = 4, 5, 30522, 8, 6, 102
    R, ld = B * K, 30528
    g = torch.Generator().manual_seed(4)
    m = beam_init(B, K, T, BOS)
    d = _to_dev(m)
    idx = torch.empty(R, K, dtype=torch.int32, device=DEV)
    lp = torch.empty(R, K, dtype=torch.float32, device=DEV)
    for i in range(steps):
        x = torch.randn(R, ld, generator=g) * 3
        if i >= 2:
            x[i::3, eos] = 14.0                                # some beams emit EOS
        if i == 4:
            x[:K, eos] = 40.0                                  # image 0 ends entirely
        xd = x.to(DEV).bfloat16()
        call("retr_topk_rows", 1, ptr(xd), ld, R, V, K, ptr(idx), ptr(lp), ops._st())
        call("retr_beam_select", ptr(idx), ptr(lp), B, K, i, T, eos, ptr(d["scores"]),
             ptr(d["finished"]), ptr(d["hist"]), ptr(d["anc"]), ptr(d["tok"]),
             ptr(d["item_done"]), ptr(d["done"]), ops._st())
        torch.cuda.synchronize()
        rt, rl = _f64_candidates(xd, V, K)
        assert torch.equal(idx.cpu(), torch.from_numpy(rt)), i
        m = beam_step(m, rt, rl.astype(np.float32), i, eos)
        h = _host(d)
        _assert_state(h, m, i, scores_exact=False)
        assert np.allclose(h["scores"].numpy(), m["scores"], rtol=0, atol=1e-5 * (i + 1)), i
    assert m["item_done"][0] == 1 and m["done"] == -1 and m["finished"][K:].any()


# ---------------------------------------------------------------- retr_topk_rows
def _topk(xd, ld, V, K, bf16):
    M = xd.shape[0]
    idx = torch.full((M, K), -1, dtype=torch.int32, device=DEV)
    lp = torch.full((M, K), float("nan"), dtype=torch.float32, device=DEV)
    call("retr_topk_rows", 1 if bf16 else 0, ptr(xd), ld, M, V, K, ptr(idx), ptr(lp), ops._st())
    torch.cuda.synchronize()
    return idx.cpu(), lp.cpu()


def _topk_reference(xd, V):
    """(order [M, V] by value descending then index ascending, float64 log-softmax [M, V]) of the
    first V columns of the device rows, as fp32 values."""
    xf = xd[:, :V].float().cpu()
    _, order = torch.sort(xf, dim=-1, descending=True, stable=True)
    return order, torch.log_softmax(xf.double(), -1)


def _check_topk(xd, ld, V, bf16, ks, atol=1e-5):
    """Every K in ks on the same rows: exact indices (never a pad column), finite log-softmax
    within atol wherever the word is finite, -inf where it is -inf."""
    order, ref_lp = _topk_reference(xd, V)
    for K in ks:
        idx, lp = _topk(xd, ld, V, K, bf16)
        assert int(idx.max()) < V and int(idx.min()) >= 0, (V, K)
        assert torch.equal(idx.long(), order[:, :K]), (V, K)
        want = ref_lp.gather(1, order[:, :K])
        fin = torch.isfinite(want)
        assert bool(torch.isfinite(lp[fin]).all()), (V, K, lp)
        assert bool((lp[~fin] == float("-inf")).all()), (V, K)
        err = (lp.double() - want)[fin].abs().max() if fin.any() else 0.0
        assert float(err) <= atol, (V, K, float(err))


def _poison_pads(x, V):
    """Columns [V, ld) are not part of the row: +1e30 in even rows, NaN in odd ones."""
    x[0::2, V:] = 1e30
    x[1::2, V:] = float("nan")
    return x


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("V", [5, 8, 1003, 32768, 32769, 32771])
def test_topk_rows_every_k_and_poisoned_pads(dtype, V):
    """K = 1 .. 8 of the register kernel (V <= 32768, incl. V = 8 = K and the tail-only V = 5) and
    of the streaming kernel (32769 and 32771: tails of 1 and 3 words), with planted ties and the
    pad columns poisoned."""
    M, ld = 8, (V + 15) // 8 * 8
    g = torch.Generator().manual_seed(V)
    x = torch.randn(M, ld, generator=g) * 3
    x[0, [1 % V, V // 2, V - 1]] = 20.0                          # ties -> ascending index
    x[1, V - 1] = 30.0                                           # the last word of the tail
    x[2, :] = 1.5                                                # a constant row: indices 0..K-1
    x[3, torch.arange(3 % V, V, max(1, V // 200))] = 25.0        # > 64 tied candidates
    if V > 64:
        x[4, 40:40 + 16] = 15.0 + torch.arange(16).float() / 4   # the best words in two chunks
    x = _poison_pads(x, V)
    xd = (x.bfloat16() if dtype == "bf16" else x).to(DEV)
    _check_topk(xd, ld, V, dtype == "bf16", range(1, min(V, 8) + 1))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("V", [1003, 32768, 32771])
def test_topk_rows_minus_inf_logits(dtype, V):
    """-inf logits (include/retr_hip.h: probability 0, ranked after every finite word in index
    order, log-probability -inf) in rows that keep at least one finite word: a masked range,
    fewer than K finite words, a single finite word, half the row masked, and the row in which a
    streaming-kernel thread meets only -inf chunks (every 256th, thread 0's) before the finite
    first word of the tail."""
    M, ld = 6, (V + 15) // 8 * 8
    g = torch.Generator().manual_seed(V + 1)
    x = torch.randn(M, ld, generator=g) * 3
    ninf = float("-inf")
    x[0, 100:900] = ninf
    x[1, :V] = ninf
    x[1, [5, 77, V - 1]] = torch.tensor([1.0, 3.0, 2.0])
    x[2, :V] = ninf
    x[2, V - 1] = -4.0
    x[3, :V][torch.rand(V, generator=g) < 0.5] = ninf
    for c in range(0, V // 8, 256):
        x[4, 8 * c:8 * c + 8] = ninf
    x[4, V // 8 * 8 - (0 if V % 8 else 1)] = 2.5                 # V = 32771: word 32768
    x[5, :V // 8 * 8] = ninf                                     # only tail words are finite
    if V % 8 == 0:
        x[5, V - 2] = 0.5
    x = _poison_pads(x, V)
    xd = (x.bfloat16() if dtype == "bf16" else x).to(DEV)
    _check_topk(xd, ld, V, dtype == "bf16", range(1, 9))


@pytest.mark.parametrize("V", [1003, 32771])
def test_topk_rows_large_magnitudes(V):
    """fp32 rows around -1e4, +1e4 and mixing both: exact indices; log-softmax within
    1e-5 + 4 ulp_fp32(max |x|) -- the project's tolerance plus the rounding of the fp32
    log-sum-exp and of the subtraction value - lse at that magnitude."""
    M, ld = 6, (V + 15) // 8 * 8
    g = torch.Generator().manual_seed(V + 2)
    x = torch.randn(M, ld, generator=g) * 3
    x[0:2] += 1e4
    x[2:4] -= 1e4
    x[4:6, 0::2] += 1e4
    x[4:6, 1::2] -= 1e4
    xd = _poison_pads(x, V).to(DEV)
    big = float(x[:, :V].abs().max())
    atol = 1e-5 + 4 * float(np.spacing(np.float32(big)))
    _check_topk(xd, ld, V, False, range(1, 9), atol=atol)
