"""numpy model of one decode-bookkeeping step, shared by the beam / greedy state tests.  Written
from the documented semantics (the header comment of csrc/beam.hip, include/retr_hip.h,
oracle/model.py beam_search and the greedy contract restated above greedy_update_kernel in
csrc/loss.hip), not from the kernels' rank / LDS logic: candidates are listed in (beam, rank)
order and the survivors are taken serially, "the first best unused candidate, K times".

State dicts hold numpy arrays; a step returns a new dict and leaves its argument untouched.
  beam:   scores f32 [R], finished u8 [R], hist i64 [R, T], anc i32 [R, T], tok i64 [R],
          item_done u8 [B], done int          (R = B * K, row b * K + k = beam k of image b)
  greedy: caption i64 [B, T], finished u8 [B], tok i64 [B], done int
"""
import numpy as np


def beam_init(B, K, T, bos):
    """The state IncrementalBeam._reset leaves: BOS in column 0, every cache row its own."""
    R = B * K
    hist = np.zeros((R, T), np.int64)
    hist[:, 0] = bos
    return dict(scores=np.zeros(R, np.float32), finished=np.zeros(R, np.uint8), hist=hist,
                anc=np.repeat(np.arange(R, dtype=np.int32)[:, None], T, 1),
                tok=np.full(R, bos, np.int64), item_done=np.zeros(B, np.uint8), done=-1)


def copy_state(state):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}


def beam_candidates(scores, finished, cand_tok, cand_lp, r0, K, i):
    """Image r0 // K's candidates in (beam, rank) order: (total fp32, parent beam, token)."""
    out = []
    for k in range(K if i > 0 else 1):               # step 0: the K rows are copies, beam 0 offers
        r = r0 + k
        if i > 0 and finished[r]:                    # one continuation, the score is kept
            out.append((np.float32(scores[r]), k, int(cand_tok[r, 0])))
            continue
        base = np.float32(scores[r]) if i > 0 else np.float32(0.0)
        for j in range(K):
            out.append((np.float32(base + np.float32(cand_lp[r, j])), k, int(cand_tok[r, j])))
    return out


def beam_step(state, cand_tok, cand_lp, i, eos):
    """One retr_beam_select call: cand_tok [R, K] int, cand_lp [R, K] float32, step i."""
    if state["done"] >= 0:                           # the decode already ended: no more writes
        return copy_state(state)
    cand_tok = np.asarray(cand_tok)
    cand_lp = np.asarray(cand_lp, dtype=np.float32)
    R, K = cand_tok.shape
    B, T = R // K, state["hist"].shape[1]
    old, new = state, copy_state(state)
    for b in range(B):
        r0 = b * K
        cands = beam_candidates(old["scores"], old["finished"], cand_tok, cand_lp, r0, K, i)
        sc = np.array([c[0] for c in cands], np.float32)
        used = np.zeros(len(cands), bool)
        for s in range(K):
            free = np.flatnonzero(~used)
            c = int(free[np.argmax(sc[free])])       # argmax: the first of equal maxima
            used[c] = True
            total, p, t = cands[c]
            new["hist"][r0 + s] = old["hist"][r0 + p]
            new["hist"][r0 + s, i + 1] = t
            new["anc"][r0 + s, :i] = old["anc"][r0 + p, :i]
            new["anc"][r0 + s, i] = r0 + p           # position i was computed in the parent's row
            new["anc"][r0 + s, i + 1:] = r0 + s
            new["scores"][r0 + s] = total
            new["finished"][r0 + s] = 1 if ((i > 0 and old["finished"][r0 + p]) or t == eos) else 0
            new["tok"][r0 + s] = t
        new["item_done"][b] = 1 if new["finished"][r0:r0 + K].all() else 0
    if new["item_done"].all():
        new["done"] = i
    return new


def best_captions(state, B, K):
    """Each image's best beam (first of equal scores), columns after the final step zero."""
    T = state["hist"].shape[1]
    best = state["scores"].reshape(B, K).argmax(-1)
    cap = state["hist"].reshape(B, K, T)[np.arange(B), best].copy()
    if state["done"] >= 0:
        cap[:, state["done"] + 1:] = 0
    return cap


def greedy_init(B, T, bos, fill=0):
    cap = np.full((B, T), fill, np.int64)
    cap[:, 0] = bos
    return dict(caption=cap, finished=np.zeros(B, np.uint8), tok=np.full(B, bos, np.int64),
                done=-1)


def greedy_step(state, pred, i, eos, write_all=False):
    """One retr_greedy_update / retr_greedy_select(2) call on the predictions of step i."""
    pred = np.asarray(pred, dtype=np.int64)
    new = copy_state(state)
    new["finished"] = (state["finished"].astype(bool) | (pred == eos)).astype(np.uint8)
    all_fin = bool(new["finished"].all())
    stop = (not write_all) and (state["done"] >= 0 or all_fin)
    if not stop:
        new["caption"][:, i + 1] = pred
    new["tok"] = pred.copy()
    if state["done"] < 0 and all_fin:
        new["done"] = i
    return new
