"""Cross entropy with ignore_index / label smoothing / reduction (retr_ce_*_opt) on the GPU.

The reference everywhere is torch.nn.functional.cross_entropy on the same, already rounded,
logits in float64 on the CPU.  Tolerances are test_cross_entropy_and_argmax's: fp32 1e-5 relative
on the loss and 5e-5 rel_err on the gradient, bf16 1e-2 and 5e-2."""
import functools

import pytest
import torch
import torch.nn.functional as F

from retr_amd import _lib, ops
from retr_amd._lib import call, ptr
from retr_amd.models.caption import CrossEntropyLoss, build_model
from retr_amd.models.utils import NestedTensor
from retr_amd.synthetic import synthetic_captions, synthetic_images, synthetic_state_dict
from tests.helpers import PARITY_CASES, make_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, T = 2, 9
M = B * T
TOL = {torch.float32: (1e-5, 5e-5), torch.bfloat16: (1e-2, 5e-2)}
NEW_CALLS = {"retr_ce_count", "retr_ce_fwd_opt", "retr_ce_bwd_opt", "retr_ce_fwd_bwd_opt",
             "retr_ce_bwd_rescale_opt"}
OLD_CALLS = {"retr_ce_fwd", "retr_ce_bwd", "retr_ce_fwd_bwd", "retr_ce_bwd_rescale"}


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _round_up(n, m):
    return (n + m - 1) // m * m


@functools.lru_cache(maxsize=None)
def _logits(V, dtype):
    """[M, Vp] device buffer (pad columns 1e4: a read past V shows up) and the float64 CPU copy
    of its rounded real columns."""
    g = torch.Generator(device="cpu").manual_seed(V)
    Vp = _round_up(V, 64)
    buf = torch.full((M, Vp), 1e4)
    buf[:, :V] = torch.randn(M, V, generator=g) * 2
    buf = buf.to(DEV).to(dtype)
    return buf, buf[:, :V].double().cpu()


@functools.lru_cache(maxsize=None)
def _targets(V, ignore):
    """(targets [M] on the CPU, ignore_index for ops.cross_entropy, ignore_index for torch)."""
    g = torch.Generator(device="cpu").manual_seed(100 + V)
    tgt = torch.randint(0, V, (M,), generator=g)
    tgt[1], tgt[3] = V - 1, 0                      # last and first column
    if ignore == "pad0":
        tgt[::2] = 0                               # every other row is the ignored class 0
        return tgt, 0, 0
    if ignore == "neg100":
        tgt[[2, 7, 12]] = -100
        return tgt, -100, -100
    return tgt, None, -100


@functools.lru_cache(maxsize=None)
def _reference(V, dtype, ignore, eps, reduction, scale):
    """float64 torch loss and gradient; the upstream gradient is `scale` (a [M] weight vector
    for reduction 'none')."""
    _, x64 = _logits(V, dtype)
    tgt, _, ii = _targets(V, ignore)
    x = x64.clone().requires_grad_(True)
    loss = F.cross_entropy(x, tgt, ignore_index=ii, label_smoothing=eps, reduction=reduction)
    (loss * _upstream(reduction, scale).double()).sum().backward()
    return loss.detach(), x.grad


def _upstream(reduction, scale):
    if reduction != "none":
        return torch.tensor(scale)
    g = torch.Generator(device="cpu").manual_seed(9)
    return torch.rand(M, generator=g) + 0.5


def _run(buf, V, tgt, ii, eps, reduction, scale, fused):
    """ops.cross_entropy forward + backward on the [B, T, V] view of `buf`.  Returns the loss and
    the padded [M, Vp] gradient buffer the backward handed to autograd."""
    Vp = buf.shape[1]
    lt = buf[:, :V].view(B, T, V).detach().requires_grad_(True)
    got = []
    lt.register_hook(got.append)
    # the kernels' output buffers come from the caching allocator: leave NaNs in what it reuses
    junk = torch.full((M, Vp), float("nan"), device=DEV, dtype=buf.dtype)
    del junk
    tg = tgt.view(B, T).to(DEV)
    if fused:
        with ops.train_step_scope():
            loss = ops.cross_entropy(lt.permute(0, 2, 1), tg, ignore_index=ii,
                                     label_smoothing=eps, reduction=reduction)
    else:
        loss = ops.cross_entropy(lt.permute(0, 2, 1), tg, ignore_index=ii, label_smoothing=eps,
                                 reduction=reduction)
    up = _upstream(reduction, scale).to(DEV)
    (loss * (up.view(B, T) if reduction == "none" else up)).sum().backward()
    torch.cuda.synchronize()
    (g,) = got
    # a view of the padded buffer: what _MLPHead.backward's fast path takes as it is
    assert g.dtype == buf.dtype and g.stride() == (T * Vp, Vp, 1)
    return loss.detach(), g.as_strided((M, Vp), (Vp, 1))


def _check(loss, grad, V, dtype, ignore, eps, reduction, scale):
    ltol, gtol = TOL[dtype]
    tgt, _, ii = _targets(V, ignore)
    lref, gref = _reference(V, dtype, ignore, eps, reduction, scale)
    ign = tgt == ii
    loss, grad = loss.double().cpu(), grad.float().cpu()
    if reduction == "none":
        loss = loss.reshape(M)
        assert torch.equal(loss[ign], torch.zeros_like(loss[ign]))
        worst = ((loss - lref).abs() / lref.abs().clamp_min(1e-30))[~ign].max().item()
        print(f"V={V} {dtype} {ignore} eps={eps} none: worst row rel {worst:.2e}")
        assert worst < ltol
    else:
        print(f"V={V} {dtype} {ignore} eps={eps} {reduction}: loss {loss.item():.7f} "
              f"ref {lref.item():.7f}")
        assert abs(loss.item() - lref.item()) < ltol * abs(lref.item())
    e = rel_err(grad[:, :V], gref)
    print(f"   grad rel_err {e:.2e}")
    assert e < gtol
    assert torch.equal(grad[ign], torch.zeros_like(grad[ign]))
    assert torch.equal(grad[:, V:], torch.zeros_like(grad[:, V:]))


# path: fp32 and bf16 through the two-pass pair, bf16 through the one-pass training form
@pytest.mark.parametrize("ignore", ["none", "pad0", "neg100"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("path", ["fp32", "bf16", "bf16_fused"])
@pytest.mark.parametrize("V", [37, 2056, 30522])
def test_kernel_grid(V, path, eps, ignore):
    dtype = torch.float32 if path == "fp32" else torch.bfloat16
    fused = path == "bf16_fused"
    buf, _ = _logits(V, dtype)
    tgt, ii, _ = _targets(V, ignore)
    for reduction in ("mean", "sum") if fused else ("mean", "sum", "none"):
        # fused: dloss = 1 keeps the forward's gradient, any other value rewrites it
        for scale in (1.0, 0.37) if fused else (0.37,):
            loss, grad = _run(buf, V, tgt, ii, eps, reduction, scale, fused)
            _check(loss, grad, V, dtype, ignore, eps, reduction, scale)


@pytest.mark.parametrize("path", ["fp32", "bf16", "bf16_fused"])
def test_all_rows_ignored(path):
    """N_valid = 0: the mean is NaN (0 / 0, as in torch), the sum 0, every gradient exactly 0."""
    V = 2056
    dtype = torch.float32 if path == "fp32" else torch.bfloat16
    buf, _ = _logits(V, dtype)
    tgt = torch.full((M,), 5)
    for reduction in ("mean", "sum"):
        loss, grad = _run(buf, V, tgt, 5, 0.1, reduction, 0.37, path == "bf16_fused")
        if reduction == "mean":
            assert torch.isnan(loss).item()
        else:
            assert loss.item() == 0.0
        assert torch.equal(grad, torch.zeros_like(grad))


@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_fused_matches_two_pass(scale):
    """test_fused_cross_entropy_matches_two_pass with options: the training step's one pass
    (retr_ce_fwd_bwd_opt + retr_ce_bwd_rescale_opt) against the two-pass pair and float64
    torch, about half the rows pad and ignored."""
    g = torch.Generator(device="cpu").manual_seed(5)
    Bf, Tf, V, Vp = 4, 33, 30522, 30528
    store = (torch.randn(Bf, Tf, Vp, generator=g) * 3).to(DEV).to(torch.bfloat16)
    tgt = torch.randint(1, V, (Bf, Tf), generator=g)
    tgt[torch.rand(Bf, Tf, generator=g) < 0.5] = 0
    crit = CrossEntropyLoss(ignore_index=0, label_smoothing=0.1)
    res = []
    try:
        for fused in (False, True):
            ops.FUSED_CE = fused
            x = store.clone().requires_grad_(True)
            with ops.train_step_scope():
                loss = crit(x[..., :V].permute(0, 2, 1), tgt.to(DEV))
            (loss * scale).backward()
            torch.cuda.synchronize()
            res.append((loss.detach().clone(), x.grad.detach().clone()))
    finally:
        ops.FUSED_CE = True
    (l0, g0), (l1, g1) = res
    xr = store[..., :V].double().cpu().requires_grad_(True)
    ref = F.cross_entropy(xr.permute(0, 2, 1), tgt, ignore_index=0, label_smoothing=0.1)
    (ref * scale).backward()
    assert abs(l1.item() - l0.item()) < 1e-5 * abs(l0.item())
    e = ((g1.float() - g0.float()).norm() / g0.float().norm()).item()
    assert e < 1e-2, e
    for l, gr in res:
        gr = gr.float().cpu()
        assert abs(l.item() - ref.item()) < 1e-2 * abs(ref.item())
        assert rel_err(gr[..., :V], xr.grad) < 5e-2
        assert torch.equal(gr[tgt == 0], torch.zeros_like(gr[tgt == 0]))
        assert torch.equal(gr[..., V:], torch.zeros_like(gr[..., V:]))


def test_denominator_is_read_on_the_device_under_graph_capture():
    """count -> fused forward + backward -> mean captured into one graph (a single chain), then
    replayed on targets with another number of ignored rows: equal to an eager run on those
    targets, which a 1 / N_valid fixed on the host at capture time could not be."""
    V, eps = 2056, 0.1
    buf, x64 = _logits(V, torch.bfloat16)
    Vp = buf.shape[1]
    tgt_a, _, _ = _targets(V, "pad0")               # every other row ignored
    tgt_b = tgt_a.clone()
    tgt_b[::2] = torch.arange(1, M // 2 + 1)
    tgt_b[4] = 0                                    # far fewer ignored rows
    assert (tgt_a == 0).sum() != (tgt_b == 0).sum()
    tgt = tgt_a.to(DEV)
    lse = torch.empty(M, device=DEV)
    rows = torch.empty(M, device=DEV)
    loss = torch.empty((), device=DEV)
    denom = torch.empty((), device=DEV)
    dl = torch.empty(M, Vp, device=DEV, dtype=torch.bfloat16)

    def sequence():
        st = _lib.stream()
        call("retr_ce_count", M, ptr(tgt), 0, ptr(denom), st)
        call("retr_ce_fwd_bwd_opt", _lib.BF16, ptr(buf), Vp, M, V, ptr(tgt), 0, eps, ptr(lse),
             ptr(rows), ptr(loss), ptr(denom), ptr(dl), Vp, st)

    # eager warm-up on the current stream: this file takes no stream from torch's pool (see
    # test_gpu_graphed_ce_options.py)
    sequence()
    torch.cuda.synchronize()
    loss_a = loss.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sequence()
    tgt.copy_(tgt_b)
    dl.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    loss_g, dl_g, n_g = loss.clone(), dl.clone(), denom.item()
    dl.fill_(float("nan"))
    sequence()
    torch.cuda.synchronize()
    assert n_g == (tgt_b != 0).sum().item()
    assert torch.equal(loss_g, loss) and torch.equal(dl_g, dl)
    assert not torch.equal(loss_g, loss_a)
    xr = x64.clone().requires_grad_(True)
    ref = F.cross_entropy(xr, tgt_b, ignore_index=0, label_smoothing=eps)
    ref.backward()
    assert abs(loss_g.item() - ref.item()) < 1e-2 * abs(ref.item())
    assert rel_err(dl_g[:, :V], xr.grad) < 5e-2


class _Recorder:
    """Stand-in for retr_amd.probe.Probe: records the name of every library call."""

    def __init__(self):
        self.names = set(_lib.exported_symbols())
        self.called = []

    def wrap(self, name, args, fn):
        self.called.append(name)
        return fn()


def test_default_criterion_keeps_its_kernels():
    """CrossEntropyLoss() calls only the four entry points it always did, bit for bit."""
    V = 2056
    rec = _Recorder()
    _lib.set_probe(rec)
    try:
        for dtype, fused in ((torch.float32, False), (torch.bfloat16, True)):
            buf, _ = _logits(V, dtype)
            tgt, _, _ = _targets(V, "none")
            lt = buf[:, :V].view(B, T, V).detach().requires_grad_(True)
            with ops.train_step_scope():
                loss = CrossEntropyLoss()(lt.permute(0, 2, 1), tgt.view(B, T).to(DEV))
            (loss * 0.5).backward()
            if not fused:
                loss_two_pass = loss.detach().clone()
        torch.cuda.synchronize()
    finally:
        _lib.set_probe(None)
    ce = {n for n in rec.called if n.startswith("retr_ce_")}
    assert ce == OLD_CALLS and not ce & NEW_CALLS
    buf, _ = _logits(V, torch.float32)
    tgt, _, _ = _targets(V, "none")
    tg = tgt.to(DEV)
    lse = torch.empty(M, device=DEV)
    rows = torch.empty(M, device=DEV)
    direct = torch.empty((), device=DEV)
    call("retr_ce_fwd", _lib.F32, ptr(buf), buf.shape[1], M, V, ptr(tg), ptr(lse), ptr(rows),
         ptr(direct), _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(loss_two_pass, direct)


@pytest.fixture(scope="module")
def micro():
    """micro_r18 in fp32 parity mode, set up as test_gpu_model._setup does, and the oracle's
    logits for its batch (with the graph for the oracle's gradients)."""
    from oracle import model as orc
    kw, size, nb = PARITY_CASES["micro_r18"]
    cfg = make_config(dtype="fp32", **kw)
    model, _ = build_model(cfg)
    sd = synthetic_state_dict(model, seed=42)
    model.load_state_dict(sd)
    model.to(DEV)
    images, mask = synthetic_images(nb, size, seed=1, pad_band=True)
    caps, cap_mask = synthetic_captions(nb, cfg.max_position_embeddings, cfg.vocab_size, seed=2)
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    sdo = {k: (v.clone().requires_grad_(True) if k in trainable else v) for k, v in sd.items()}
    lo = orc.caption_forward(sdo, cfg, images, mask, caps[:, :-1], cap_mask[:, :-1])
    return model, sdo, lo, images, mask, caps, cap_mask


def test_model_with_options_matches_oracle(micro):
    model, sdo, lo, images, mask, caps, cap_mask = micro
    model.train()
    model.zero_grad()
    crit = CrossEntropyLoss(ignore_index=0, label_smoothing=0.1)
    out = model(NestedTensor(images.to(DEV), mask.to(DEV)), caps[:, :-1].to(DEV),
                cap_mask[:, :-1].to(DEV))
    loss = crit(out.permute(0, 2, 1), caps[:, 1:].to(DEV))
    loss.backward()
    loss_o = F.cross_entropy(lo.permute(0, 2, 1), caps[:, 1:], ignore_index=0,
                             label_smoothing=0.1)
    loss_o.backward(retain_graph=True)
    assert (caps[:, 1:] == 0).any() and (caps[:, 1:] != 0).any()
    assert abs(loss.item() - loss_o.item()) <= 1e-3 * abs(loss_o.item())
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        g, go = p.grad, sdo[n].grad
        assert g is not None and go is not None, n
        denom = go.norm().item()
        if denom == 0:
            continue
        e = ((g.double().cpu() - go.double()).norm() / denom).item()
        assert e < 2e-3, (n, e)


def test_score_expressions(micro):
    from retr_amd.eval_utils.score import score_expressions
    model, _, lo, images, mask, caps, cap_mask = micro
    model.train()                                   # scoring switches to eval mode and back
    tok, seq, n = score_expressions([NestedTensor(images.to(DEV), mask.to(DEV))], model,
                                    caps.to(DEV), cap_mask.to(DEV))
    assert model.training
    Bm, Tm = caps.shape[0], caps.shape[1] - 1
    assert tok.shape == (Bm, Tm) and seq.shape == (Bm,) and n.shape == (Bm,)
    masked = cap_mask[:, 1:]
    ref = F.log_softmax(lo.detach().double(), -1).gather(2, caps[:, 1:, None]).squeeze(2)
    tok = tok.double().cpu()
    assert ((tok - ref)[~masked].abs().max() < 1e-3 * ref[~masked].abs().max()).item()
    assert torch.equal(tok[masked], torch.zeros_like(tok[masked]))
    torch.testing.assert_close(seq.double().cpu(), tok.sum(1), rtol=1e-6, atol=0)
    assert torch.equal(n.cpu(), (~masked).sum(1))
