"""numpy restatement of the retr_sample_rows contract (include/retr_hip.h), shared by the
sampling tests.  Temperature scaling is fp32 (as the kernel's); the probabilities, their
cumulative sums, the Gumbel noise and the perturbed scores are float64."""
import numpy as np

_M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def retr_hash(seed, idx):
    """The library's 64 -> 32-bit counter hash (csrc/common.hpp) of (seed, idx): ``seed`` a
    Python int (taken mod 2^64), ``idx`` an int or an integer array; np.uint64 arithmetic wraps."""
    with np.errstate(over="ignore"):
        s = np.uint64(seed & _M64)
        i = np.asarray(idx).astype(np.uint64)
        z = s * np.uint64(GOLDEN) + i * np.uint64(0xD1B54A32D192ED03) + np.uint64(0x632BE59BD9B4E019)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return (z >> np.uint64(32)).astype(np.uint32)


def stream_key(seed, draw):
    """s = seed ^ (draw * 0x9E3779B97F4A7C15), 64-bit wrapping; draw = step * M + row."""
    return (seed & _M64) ^ ((draw * GOLDEN) & _M64)


def order_of(z):
    """Indices by z descending, then index ascending."""
    return np.argsort(-z, kind="stable")


def kept_prefix(x, inv_t, top_k, top_p):
    """(z fp32, order, n_kept, q) of one row: q = float64 probabilities of the ordered top-k set."""
    z = np.asarray(x, dtype=np.float32) * np.float32(inv_t)
    V = z.shape[0]
    order = order_of(z)
    nk = V if top_k <= 0 or top_k >= V else int(top_k)
    zk = z[order[:nk]].astype(np.float64)
    q = np.exp(zk - zk[0])
    q /= q.sum()
    n = nk
    if top_p < 1.0:
        n = min(nk, int(np.searchsorted(np.cumsum(q), top_p, side="left")) + 1)
    return z, order, n, q


def ref_row(x, inv_t, top_k, top_p, seed, draw, masses=False):
    """(token, n_kept, margin) of one logits row; margin = the gap between the best and the
    second-best perturbed score (inf with a single kept word).  With ``masses`` also the
    float64 mass of the first n_kept and of the first n_kept - 1 words of the top-k set."""
    z, order, n, q = kept_prefix(x, inv_t, top_k, top_p)
    kept = np.sort(order[:n])                       # ascending index: argmax takes the lowest
    h = retr_hash(stream_key(seed, draw), kept)
    u = ((h >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    score = z[kept].astype(np.float64) - np.log(-np.log(u))
    best = int(np.argmax(score))
    margin = np.inf
    if n > 1:
        top2 = np.partition(score, n - 2)[n - 2:]
        margin = float(top2[1] - top2[0])
    out = (int(kept[best]), n, margin)
    if masses:
        out += (float(q[:n].sum()), float(q[:n - 1].sum()))
    return out


def planted_nucleus_row(V):
    """A row with probabilities {0.5, 0.3, 0.15, 0.05} at four indices and logit -30 elsewhere;
    returns (logits fp32, {top_p: expected n_kept}).  No top_p listed sits on a boundary of the
    cumulative masses 0.5 / 0.8 / 0.95 / 1."""
    x = np.full(V, -30.0, dtype=np.float32)
    for j, p in zip((V // 2, 3, V - 1, V // 3), (0.5, 0.3, 0.15, 0.05)):
        x[j] = np.float32(np.log(p))
    return x, {0.4: 1, 0.7: 2, 0.9: 3, 0.97: 4}
