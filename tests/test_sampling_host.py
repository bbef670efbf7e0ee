"""Sampling decode, the parts that need no GPU: argument checking of ``sample`` (raised before
any GPU work), the numpy reference of the retr_sample_rows contract itself (tests/
sampling_ref.py: its draws follow softmax, its nucleus cut is exact on a planted row), and the
entry point's declaration in the C-ABI header."""
import ctypes

import numpy as np
import pytest

from tests.sampling_ref import kept_prefix, planted_nucleus_row, ref_row, retr_hash


@pytest.mark.parametrize("kw", [
    dict(temperature=-0.5), dict(temperature=float("nan")), dict(temperature=float("inf")),
    dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5),
    dict(top_p=float("nan")), dict(num_samples=0), dict(num_samples=-2)])
def test_invalid_arguments_raise_before_gpu_work(kw):
    from retr_amd.eval_utils.decode import IncrementalSampler, sample
    with pytest.raises(ValueError):
        sample([], None, **kw)           # no model, no samples: nothing but the check may run
    with pytest.raises(ValueError):
        IncrementalSampler(None, **kw)


def test_hash_restatement_known_values():
    """np.uint64 restatement == the same formula in Python integers (mod 2^64)."""
    M = (1 << 64) - 1

    def h(seed, idx):
        z = (seed * 0x9E3779B97F4A7C15 + idx * 0xD1B54A32D192ED03 + 0x632BE59BD9B4E019) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        return z >> 32
    idx = np.array([0, 1, 63, 30521, 2 ** 31 - 1])
    for seed in (0, 1, 12345, M, 0x9E3779B97F4A7C15, -7):
        got = retr_hash(seed, idx)
        assert got.dtype == np.uint32
        assert got.tolist() == [h(seed & M, int(i)) for i in idx]


def test_reference_draws_follow_softmax():
    """20000 draws (draw index 0..19999, temperature 1, no filter) of one fixed 64-word row:
    every word's count within 5 sigma of N * softmax; another seed gives another sequence."""
    V, N = 64, 20000
    x = (1.5 * np.random.default_rng(3).standard_normal(V)).astype(np.float32)
    p = np.exp(x.astype(np.float64) - x.max())
    p /= p.sum()
    toks = {seed: np.array([ref_row(x, 1.0, 0, 1.0, seed, d)[0] for d in range(N)])
            for seed in (1234, 99)}
    for seed, t in toks.items():
        counts = np.bincount(t, minlength=V)
        sigma = np.sqrt(N * p * (1 - p))
        zscore = np.abs(counts - N * p) / sigma
        assert zscore.max() < 5.0, (seed, float(zscore.max()))
    assert (toks[1234] != toks[99]).any()
    n_kept = ref_row(x, 1.0, 0, 1.0, 1234, 0)[1]
    assert n_kept == V


def test_reference_order_topk_and_greedy():
    x = np.array([0.5, 2.0, -1.0, 2.0, 0.5, 2.0, -np.inf, 1.0], dtype=np.float32)
    z, order, n, q = kept_prefix(x, 1.0, 4, 1.0)
    assert order.tolist() == [1, 3, 5, 7, 0, 4, 2, 6]        # value desc, index asc on ties
    assert n == 4 and abs(q.sum() - 1.0) < 1e-12
    for k, want in ((0, 8), (8, 8), (100, 8), (2, 2)):
        assert kept_prefix(x, 1.0, k, 1.0)[2] == want
    for seed in range(20):                                   # top_k = 1: the first-index argmax
        assert ref_row(x, 0.7, 1, 1.0, seed, seed)[:2] == (1, 1)
        assert ref_row(x, 1.0, 2, 1.0, seed, 0)[0] in (1, 3)  # planted tie: the lower indices
        assert ref_row(x, 1.0, 0, 1.0, seed, 0)[0] != 6       # -inf is never drawn


@pytest.mark.parametrize("V", [64, 1003, 30522])
def test_reference_planted_nucleus(V):
    x, expected = planted_nucleus_row(V)
    for top_p, n in expected.items():
        assert kept_prefix(x, 1.0, 0, top_p)[2] == n, top_p
        assert ref_row(x, 1.0, 0, top_p, 5, 0)[1] == n
    assert kept_prefix(x, 1.0, 2, 0.9)[2] == 2               # renormalised over the top-2 set
    assert kept_prefix(x, 1.0, 2, 0.6)[2] == 1               # 0.5 / 0.8 = 0.625 >= 0.6


def test_entry_point_is_declared():
    from retr_amd import _lib
    restype, params = _lib.FUNCTIONS["retr_sample_rows"]
    assert restype is ctypes.c_int
    p, i, lng = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert params == [("dtype", i), ("logits", p), ("ld", lng), ("M", i), ("V", i),
                      ("fparams", p), ("iparams", p), ("step", i), ("finished", p),
                      ("pred", p), ("logprob", p), ("n_kept", p), ("stream", p)]
