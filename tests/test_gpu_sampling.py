"""Sampling decode on the KV-cache path: the retr_sample_rows kernel (csrc/sample.hip) against
the numpy restatement of its contract (tests/sampling_ref.py), and IncrementalSampler /
``sample`` against greedy (the parity anchor), eager launches, the per-step reference and
``score_expressions``.

Token equality with the reference leaves out the rows whose best two perturbed scores are
closer than NEAR_TIE: there fp32 logf and the rounding of z + g may legitimately pick the other
word.  At most MAX_LEFT_OUT of a case's rows may be left out (the reference leaves out <= 1 of
256 on these inputs); more is a failure of the test inputs, not a pass."""
import functools

import numpy as np
import pytest
import torch

from retr_amd import ops
from retr_amd._lib import call, ptr
from retr_amd.eval_utils.decode import IncrementalSampler, greedy, sample
from retr_amd.eval_utils.score import score_expressions
from retr_amd.models.caption import build_model
from retr_amd.models.utils import NestedTensor
from retr_amd.synthetic import synthetic_images, synthetic_state_dict
from tests.helpers import PARITY_CASES, make_config
from tests.sampling_ref import kept_prefix, planted_nucleus_row, ref_row

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 256
STEP = 3                        # a decode step > 0: draw = STEP * M + row
NEAR_TIE = 1e-3
MAX_LEFT_OUT = 0.02
# (temperature, top_k, top_p) and the seed used with each
PARAMS = [(1.0, 0, 1.0), (0.7, 50, 1.0), (0.7, 0, 0.9), (1.3, 40, 0.95), (1.0, 1, 1.0)]
SEEDS = [12345, -7, 2 ** 62 + 3, 0x1234567, 99]
FINISHED_EVERY = 5              # rows r % 5 == 2 enter the kernel finished


def _inv_t(temperature):
    return np.float32(1.0) / np.float32(temperature)


def _plant_kth_ties(x, row, k):
    """k - 3 distinct values above five words tied at 20.0: the ties take places k-2 .. k+2 of
    the order, so top-k keeps the three with the lowest indices (5, 301, 302)."""
    hi = torch.arange(k - 3) * 2 + 100
    x[row, hi] = 25.0 + torch.arange(k - 3).float() / 64
    x[row, torch.tensor([5, 301, 302, 640, 999])] = 20.0


@functools.lru_cache(maxsize=2)
def _logits(dtype, V):
    """(logits [M, ld] in ``dtype`` on the CPU, the same as fp32 numpy [M, V], float64
    log-sum-exp per row): 3 * randn with planted rows; columns >= V hold a large value that
    must never be a candidate."""
    ld = (V + 15) // 8 * 8
    g = torch.Generator().manual_seed(2 * V + (dtype == "bf16"))
    x = torch.randn(M, ld, generator=g) * 3
    _plant_kth_ties(x, 0, 50)
    _plant_kth_ties(x, 4, 40)
    # 35 tied best words: fewer than either k, and neither 0.9 * 35 nor 0.95 * 35 is near an
    # integer, so no nucleus of the parameter sets ends on a boundary of this row
    x[1, torch.arange(7, V, V // 35)[:35]] = 25.0
    x[2, V - 1] = 30.0                                           # last (partial) chunk
    x[3, 10:20] = -float("inf")                                  # probability 0
    x[:, V:] = 50.0
    t = x.bfloat16() if dtype == "bf16" else x
    xf = t.float()[:, :V].contiguous()
    lse = torch.logsumexp(xf.double(), -1).numpy()
    return t, xf.numpy(), lse


@functools.lru_cache(maxsize=None)
def _reference(dtype, V, pidx):
    """Per row of _logits(dtype, V) under PARAMS[pidx] / SEEDS[pidx]: token, n_kept, margin,
    mass of the first n_kept / n_kept - 1 words.  Computed once, never modified."""
    _, xf, _ = _logits(dtype, V)
    temperature, k, p = PARAMS[pidx]
    rows = [ref_row(xf[r], _inv_t(temperature), k, p, SEEDS[pidx], STEP * M + r, masses=True)
            for r in range(M)]
    out = tuple(np.array(c) for c in zip(*rows))
    for a in out:
        a.setflags(write=False)
    return out


def _device_params(pidx):
    temperature, k, p = PARAMS[pidx]
    seed = (SEEDS[pidx] + 2 ** 63) % 2 ** 64 - 2 ** 63
    return (torch.tensor([_inv_t(temperature), p], dtype=torch.float32),
            torch.tensor([k, seed], dtype=torch.int64))


def _launch(xd, V, dtype, fp, ip, fin, step=STEP):
    rows, ld = xd.shape
    pred = torch.full((rows,), -1, dtype=torch.long, device=DEV)
    lp = torch.full((rows,), 7.0, dtype=torch.float32, device=DEV)
    nk = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    call("retr_sample_rows", 1 if dtype == "bf16" else 0, ptr(xd), ld, rows, V, ptr(fp), ptr(ip),
         step, ptr(fin), ptr(pred), ptr(lp), ptr(nk), ops._st())
    torch.cuda.synchronize()
    return pred.cpu().numpy(), lp.cpu().numpy(), nk.cpu().numpy()


def _check_tokens(pred, ref_tok, margin, what):
    sure = margin >= NEAR_TIE
    left_out = 1.0 - sure.mean()
    print(f"{what}: {int((~sure).sum())} of {len(sure)} rows near a tie, "
          f"{int((pred[sure] != ref_tok[sure]).sum())} mismatches")
    assert left_out <= MAX_LEFT_OUT, (what, left_out)
    bad = np.nonzero(pred[sure] != ref_tok[sure])[0]
    assert bad.size == 0, (what, bad[:8], pred[sure][bad[:8]], ref_tok[sure][bad[:8]])


@pytest.mark.parametrize("pidx", range(len(PARAMS)))
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("V", [1003, 30522, 40000])
def test_sample_rows_matches_reference(V, dtype, pidx):
    """V 1003: ragged tail; 30522: the register-resident path; 40000: the streaming path."""
    temperature, k, p = PARAMS[pidx]
    t, xf, lse = _logits(dtype, V)
    tok, n_ref, margin, mass_n, mass_nm1 = _reference(dtype, V, pidx)
    xd = t.to(DEV)
    fp, ip = (a.to(DEV) for a in _device_params(pidx))
    fin_h = (torch.arange(M) % FINISHED_EVERY == 2)
    fin = fin_h.to(torch.uint8).to(DEV)
    pred, lp, nk = _launch(xd, V, dtype, fp, ip, fin)
    assert pred.min() >= 0 and pred.max() < V

    # membership: pred is among the first n_kept words by (z desc, index asc)
    z = xf * _inv_t(temperature)
    zp = z[np.arange(M), pred][:, None]
    j = np.arange(V)[None, :]
    rank = (z > zp).sum(1) + ((z == zp) & (j < pred[:, None])).sum(1)
    assert (rank < nk).all(), np.nonzero(rank >= nk)[0][:8]
    assert np.isfinite(xf[np.arange(M), pred]).all()             # -inf is never drawn

    nk_topk = V if k <= 0 or k >= V else k
    if p >= 1.0:
        # top-k is exact integer logic (rows 0 and 4 hold ties across the k-th place; which of
        # them are kept shows in the token equality below and, drawn on purpose, in
        # test_topk_ties_keep_the_lower_indices)
        assert (nk == nk_topk).all(), nk[nk != nk_topk][:8]
    else:
        # nucleus: mass(first n) >= top_p - tol, and n == 1 or mass(first n-1) < top_p + tol;
        # tol = V * 2^-23: any-order fp32 summation of V non-negative terms, (V-1) * 2^-24
        # relative, doubled for the rounding of each exp
        tol = V * 2.0 ** -23
        for r in range(M):
            n = int(nk[r])
            assert 1 <= n <= nk_topk, (r, n)
            if n == n_ref[r]:
                m_n, m_nm1 = mass_n[r], mass_nm1[r]
            else:
                q = kept_prefix(xf[r], _inv_t(temperature), k, p)[3]
                m_n, m_nm1 = q[:n].sum(), q[:n - 1].sum()
            assert m_n >= p - tol, (r, n, n_ref[r], m_n)
            assert n == 1 or m_nm1 < p + tol, (r, n, n_ref[r], m_nm1)

    _check_tokens(pred, tok, margin, f"V {V} {dtype} {PARAMS[pidx]}")

    if k == 1:      # the first-index argmax of the logits, on every row
        am = torch.empty(M, dtype=torch.long, device=DEV)
        call("retr_argmax_rows", 1 if dtype == "bf16" else 0, ptr(xd), xd.shape[1], M, V,
             ptr(am), ops._st())
        torch.cuda.synchronize()
        assert np.array_equal(pred, am.cpu().numpy())
        assert (nk == 1).all()

    # log-softmax of the RAW logits at pred; exactly 0 on the rows that entered finished
    want = xf[np.arange(M), pred].astype(np.float64) - lse
    live = ~fin_h.numpy()
    assert np.abs(lp[live] - want[live]).max() <= 1e-5, np.abs(lp[live] - want[live]).max()
    assert (lp[~live] == 0).all()

    # run to run: the same bits
    pred2, lp2, nk2 = _launch(xd, V, dtype, fp, ip, fin)
    assert np.array_equal(pred, pred2) and np.array_equal(nk, nk2)
    assert np.array_equal(lp.view(np.uint32), lp2.view(np.uint32))

    # the parameters are read from the device: overwritten in place, same host arguments
    nxt = (pidx + 1) % len(PARAMS)
    fp2, ip2 = _device_params(nxt)
    fp.copy_(fp2)
    ip.copy_(ip2)
    pred3, _, nk3 = _launch(xd, V, dtype, fp, ip, fin)
    tok3, n3 = _reference(dtype, V, nxt)[:2]
    _check_tokens(pred3, tok3, _reference(dtype, V, nxt)[2], f"-> {PARAMS[nxt]}")
    if PARAMS[nxt][2] >= 1.0:
        assert np.array_equal(nk3, n3)


@pytest.mark.parametrize("n_ties,k", [(8, 5), (100, 70)])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("V", [1003, 30522, 40000])
def test_topk_ties_keep_the_lower_indices(V, dtype, n_ties, k):
    """n_ties words tied at the best value, top_k = k < n_ties: only the k with the lowest
    indices are ever drawn (with 8 ties and k = 5, over 256 draws -- one per row -- each of the
    five is), and the drawn words are the reference's."""
    ties = sorted({3, 64, 65, 500, 777, 800, 901, V - 1} |
                  set(range(130, 130 + 9 * (n_ties - 8), 9)))
    assert len(ties) == n_ties and ties[-1] == V - 1
    x = torch.randn(M, (V + 15) // 8 * 8, generator=torch.Generator().manual_seed(V)) * 3
    x[:, ties] = 20.0
    x[:, V:] = 50.0
    t = x.bfloat16() if dtype == "bf16" else x
    fp = torch.tensor([1.0, 1.0], dtype=torch.float32, device=DEV)
    ip = torch.tensor([k, 424242], dtype=torch.int64, device=DEV)
    pred, _, nk = _launch(t.to(DEV), V, dtype, fp, ip, None)
    assert (nk == k).all()
    assert set(pred.tolist()) <= set(ties[:k])
    if k == 5:
        assert set(pred.tolist()) == set(ties[:k])
    xf = t.float()[:, :V].numpy()
    rows = range(0, M, 4)
    want = [ref_row(xf[r], 1.0, k, 1.0, 424242, STEP * M + r) for r in rows]
    _check_tokens(pred[::4], np.array([w[0] for w in want]), np.array([w[2] for w in want]),
                  f"ties V {V} {dtype} k {k}")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("V", [1003, 30522])
def test_planted_nucleus_is_exact(V, dtype):
    """Probabilities {0.5, 0.3, 0.15, 0.05}: n_kept is exactly 1, 2, 3, 4 at top_p 0.4, 0.7,
    0.9, 0.97 (no top_p near a boundary, so no tolerance)."""
    x, expected = planted_nucleus_row(V)
    ld = (V + 15) // 8 * 8
    rows = torch.full((3, ld), 50.0)
    rows[:, :V] = torch.from_numpy(x)
    t = (rows.bfloat16() if dtype == "bf16" else rows).to(DEV)
    xf = t.float().cpu().numpy()[0, :V]
    for top_p, n in expected.items():
        assert kept_prefix(xf, 1.0, 0, top_p)[2] == n            # also after bf16 rounding
        fp = torch.tensor([1.0, top_p], dtype=torch.float32, device=DEV)
        ip = torch.tensor([0, 77], dtype=torch.int64, device=DEV)
        pred, lp, nk = _launch(t, V, dtype, fp, ip, None, step=0)
        assert nk.tolist() == [n] * 3, (top_p, nk)
        order = kept_prefix(xf, 1.0, 0, top_p)[1]
        assert set(pred.tolist()) <= set(order[:n].tolist())


# ---- the decoder ------------------------------------------------------------------------------

def _setup(case, dtype="fp32"):
    kw, size, B = PARITY_CASES[case]
    cfg = make_config(dtype=dtype, **kw)
    model, _ = build_model(cfg)
    sd = synthetic_state_dict(model, seed=42)
    model.load_state_dict(sd)
    model.to(DEV).eval()
    images, mask = synthetic_images(B, size, seed=1, pad_band=True)
    return cfg, model, images, mask


@pytest.fixture(scope="module")
def micro():
    cfg, model, images, mask = _setup("micro_r18")
    samples = [NestedTensor(images.to(DEV), mask.to(DEV))]
    return cfg, model, samples, cfg.max_position_embeddings


BOS = 101


def test_greedy_parity(micro):
    """top_k = 1 and temperature = 0 are greedy, token for token, with graphs on: EOS never,
    mid-sequence, and at step 1 (early exit)."""
    cfg, model, samples, T = micro
    never = greedy(samples, model, max_len=T, bos_token=BOS, eos_token=-1)
    for eos in (-1, int(never[0, 6]), int(never[0, 1])):
        g = greedy(samples, model, max_len=T, bos_token=BOS, eos_token=eos)
        s1 = sample(samples, model, max_len=T, top_k=1, seed=5, bos_token=BOS, eos_token=eos)
        s0 = sample(samples, model, max_len=T, temperature=0, top_p=0.5, seed=6, bos_token=BOS,
                    eos_token=eos)
        assert torch.equal(g, s1) and torch.equal(g, s0), eos


def test_graph_replay_equals_eager(micro):
    cfg, model, samples, T = micro
    for params in ((1.0, 0, 1.0), (0.8, 20, 0.9)):
        dg = IncrementalSampler(model, *params, seed=11)
        de = IncrementalSampler(model, *params, seed=11, use_graphs=False)
        ids_g, ids_e = dg(samples, T, BOS, -1), de(samples, T, BOS, -1)
        assert torch.equal(ids_g, ids_e)
        assert torch.equal(dg.last_token_logprobs.view(torch.int32),
                           de.last_token_logprobs.view(torch.int32))
        assert bool((dg.last_token_logprobs <= 0).all())


def test_seed_reproducibility(micro):
    cfg, model, samples, T = micro
    kw = dict(max_len=T, temperature=1.0, bos_token=BOS, eos_token=-1)
    a = sample(samples, model, seed=1, **kw)
    assert torch.equal(a, sample(samples, model, seed=1, **kw))
    assert not torch.equal(a, sample(samples, model, seed=2, **kw))
    torch.manual_seed(7)                    # seed=None: torch's default CPU generator
    b = sample(samples, model, **kw)
    torch.manual_seed(7)
    assert torch.equal(b, sample(samples, model, **kw))


def _sampler_state(model):
    sts = [st for key, st in model._retr_decode_states.items() if key[0] == "IncrementalSampler"]
    assert len(sts) == 1
    return sts[0]


def test_no_recapture_when_parameters_change():
    """One captured graph serves every setting: the parameters live in device memory."""
    cfg, model, images, mask = _setup("micro_r18")       # a model of its own: one sampler state
    samples = [NestedTensor(images.to(DEV), mask.to(DEV))]
    T = cfg.max_position_embeddings
    g = greedy(samples, model, max_len=T, bos_token=BOS, eos_token=-1)
    dec = IncrementalSampler(model, 1.0, 0, 1.0, seed=3)
    first = dec(samples, T, BOS, -1)
    graphs = _sampler_state(model).graphs
    assert graphs
    dec.top_k = 1
    assert torch.equal(dec(samples, T, BOS, -1), g)
    assert _sampler_state(model).graphs is graphs
    dec.top_k = 0
    assert torch.equal(dec(samples, T, BOS, -1), first)
    assert _sampler_state(model).graphs is graphs
    dec.seed = 4
    assert not torch.equal(dec(samples, T, BOS, -1), first)
    assert _sampler_state(model).graphs is graphs


class _Recording(IncrementalSampler):
    """Keeps every step's logits (eager launches only)."""

    def _select(self, st, i, V, eos_token, s):
        self.steps.append(st.logits[:, :V].float().clone())
        super()._select(st, i, V, eos_token, s)


def test_draw_indexing_end_to_end(micro):
    """Replaying the reference over the recorded per-step logits with draw = i * R + row gives
    every written token (R = 8 rows: 4 samples of each of the 2 images)."""
    cfg, model, samples, T = micro
    temperature, k, p, seed = 0.9, 100, 0.95, 2024
    dec = _Recording(model, temperature, k, p, num_samples=4, seed=seed, use_graphs=False)
    dec.steps = []
    ids = dec(samples, T, BOS, -1).cpu().numpy()
    R = ids.shape[0]
    assert R == 8 and len(dec.steps) == T - 1
    got, want, margin = [], [], []
    for i, logits in enumerate(dec.steps):
        x = logits.cpu().numpy()
        for r in range(R):
            tok, _, mg = ref_row(x[r], _inv_t(temperature), k, p, seed, i * R + r)
            got.append(ids[r, i + 1]), want.append(tok), margin.append(mg)
    _check_tokens(np.array(got), np.array(want), np.array(margin), "decode steps")


def test_logprobs_agree_with_scoring(micro):
    """token / sequence log-probabilities of the drawn captions == score_expressions on them
    (caption mask from the first EOS), within 2e-3 * max|logits| per token: twice the relative
    logit tolerance smoke() grants the GPU forward, since a log-softmax moves by at most twice
    the largest logit error."""
    cfg, model, samples, T = micro
    kw = dict(max_len=T, temperature=1.0, top_k=0, top_p=1.0, seed=21, bos_token=BOS)
    never = sample(samples, model, eos_token=-1, **kw)
    for eos in (-1, int(never[0, 6])):
        dec = IncrementalSampler(model, 1.0, 0, 1.0, seed=21)
        ids = dec(samples, T, BOS, eos)
        ids2, tok_lp, seq_lp = sample(samples, model, eos_token=eos, return_logprobs=True, **kw)
        assert torch.equal(ids, ids2) and torch.equal(tok_lp, dec.last_token_logprobs)
        R = ids.shape[0]
        assert tok_lp.shape == (R, T - 1) and seq_lp.shape == (R,)
        # column c of ids counts if it was written (c <= the step that ended the decode) and
        # lies at or before the row's first EOS
        col = torch.arange(T, device=DEV)[None, :]
        is_eos = ids == eos
        first = torch.where(is_eos.any(1), is_eos.int().argmax(1), torch.full((R,), T, device=DEV))
        masked = col > first[:, None]
        if dec.last_done >= 0:
            masked |= col > dec.last_done
        caps = torch.cat([ids, torch.zeros(R, 1, dtype=ids.dtype, device=DEV)], 1)
        cap_masks = torch.cat([masked, torch.ones(R, 1, dtype=torch.bool, device=DEV)], 1)
        ref_tok, ref_seq, _ = score_expressions(samples, model, caps, cap_masks)
        with torch.no_grad():
            scale = float(model(*samples, ids, masked).abs().max())
        live = ~masked[:, 1:]
        err = (tok_lp - ref_tok[:, :T - 1]).abs()
        print(f"eos {eos}: max token log-prob error {float(err[live].max()):.3e}, "
              f"bound {2e-3 * scale:.3e}")
        assert float(err[live].max()) <= 2e-3 * scale
        assert bool((tok_lp[~live] == 0).all())
        assert float((seq_lp - ref_seq).abs().max()) <= 2e-3 * scale * (T - 1)
        assert torch.allclose(seq_lp, tok_lp.sum(1))


def test_multiple_samples_per_image(micro):
    """num_samples = 3: [3B, T], image-major.  Row 3b + s of that call draws with the counter
    step * 3B + (3b + s) of the seed's stream, so it equals row 3b + s of a num_samples = 1 call
    with the SAME seed on a batch of 3B images that holds image b in slot 3b + s: three such
    calls (s = 0, 1, 2), each with every other slot holding the other image."""
    cfg, model, samples, T = micro
    nt = samples[0]
    images, mask = nt.tensors, nt.mask
    B, n = images.shape[0], 3
    kw = dict(max_len=T, temperature=1.0, seed=77, bos_token=BOS, eos_token=-1)
    ids = sample(samples, model, num_samples=n, **kw)
    assert ids.shape == (n * B, T) and bool((ids[:, 0] == BOS).all())
    assert not torch.equal(ids[0], ids[1])                       # the samples are not copies
    for s in range(n):
        slot_image = torch.tensor([(r // n) if r % n == s else (r // n + 1) % B
                                   for r in range(n * B)], device=DEV)
        one = sample([NestedTensor(images[slot_image], mask[slot_image])], model, **kw)
        for b in range(B):
            assert torch.equal(one[n * b + s], ids[n * b + s]), (b, s)


def test_sample_cfg5_shape_bf16():
    """cfg5 decode shape (R50 dil 224, 6/6 d256, V 30522, T 128, batch 64) in bf16: top_k = 1
    is greedy bitwise; a nucleus run replays as the eager launches; tokens in range;
    log-probabilities finite and <= 0."""
    kw = dict(backbone="ResNet50", dilation=True, hidden=256, layers=(6, 6), vocab=30522,
              max_pos=128, ffn=2048)
    cfg = make_config(dtype="bf16", **kw)
    model, _ = build_model(cfg)
    model.load_state_dict(synthetic_state_dict(model, seed=42))
    model.to(DEV).eval()
    B, T, V = 64, 128, 30522
    images, mask = synthetic_images(B, 224, seed=7)
    samples = [NestedTensor(images.to(DEV), mask.to(DEV))]
    g = greedy(samples, model, max_len=T, bos_token=101, eos_token=102)
    s1 = sample(samples, model, max_len=T, top_k=1, seed=1, bos_token=101, eos_token=102)
    assert torch.equal(g, s1)
    dg = IncrementalSampler(model, 0.7, 0, 0.9, seed=9)
    de = IncrementalSampler(model, 0.7, 0, 0.9, seed=9, use_graphs=False)
    a, b = dg(samples, T, 101, 102), de(samples, T, 101, 102)
    assert torch.equal(a, b)
    assert torch.equal(dg.last_token_logprobs.view(torch.int32),
                       de.last_token_logprobs.view(torch.int32))
    assert a.shape == (B, T) and bool((a[:, 0] == 101).all())
    assert int(a.min()) >= 0 and int(a.max()) < V
    lp = dg.last_token_logprobs
    assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())
