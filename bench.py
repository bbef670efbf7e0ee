"""RE⫶TR hot-path benchmark on MI355X (BASELINE.json metric).

Step = one reference training step (engine.py:70-83): Caption forward, CrossEntropy, backward,
RCCL gradient all-reduce (N>1, overlapped with backward), clip_grad_norm_(0.1), AdamW — on
BASELINE config 2 (ResNet-50 + 6/6 encoder/decoder, d_model 256, 640x640 RefCOCO-shaped
synthetic batch of 16 per GPU, bf16 operands / fp32 master weights, dropout 0.1), or with
``--workload cfg4`` the per-GPU slice of config 4 (ResNet-101 + 6/6, d_model 512, 800x800,
batch 8).  A plain run sets up, warms up, times the K steps and prints the result line; with
``--dump-outputs DIR`` it also writes what the last timed step left its caller (the loss and the
norms of the updated parameters) as DIR/<name>.npy.  ``--full`` adds everything else that is reported: the
per-kernel probe and roofline (an eager re-run of the step), greedy-decode refs/sec on config 5
(ResNet-50 dilation=True 224x224, batch 64, 127 steps) in bf16 and in fp32 parity mode, beam 5,
and the CPU oracle timed on this host's cores (training step and the reference decode algorithm).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cfg2|cfg4] [--full]
                    [--dump-outputs DIR]
    torchrun --nproc-per-node N bench.py --gpus N ...    (one process per GPU, RCCL)
Rank 0 prints one JSON line.
"""
import argparse
import datetime
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from retr_amd.configuration import Config  # noqa: E402
from retr_amd.models.caption import build_model  # noqa: E402
from retr_amd.models.utils import NestedTensor  # noqa: E402
from retr_amd.synthetic import (synthetic_captions, synthetic_images,  # noqa: E402
                                synthetic_state_dict)
from retr_amd import probe as probe_mod  # noqa: E402

# Collective timeout of the bench's process group: every rank runs the same build / capture /
# timed loop, so no collective legitimately waits long; a deadlocked multi-rank run (a schedule
# disagreement the pre-flight missed, a lost rank) then fails within minutes instead of holding
# the node for NCCL's default 10 minutes per collective.
DIST_TIMEOUT = datetime.timedelta(minutes=2)

METRIC = "RefCOCO images/sec (train fwd+bwd) at 1/2/4/8 GPUs; greedy-decode refs/sec"
PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0


def cfg2(dtype="bf16"):
    c = Config()
    c.backbone, c.dilation, c.hidden_dim = "ResNet50", False, 256
    c.enc_layers = c.dec_layers = 6
    c.nheads, c.dim_feedforward, c.dropout = 8, 2048, 0.1
    c.lr_backbone, c.lr, c.weight_decay = 1e-5, 1e-4, 1e-4
    c.dtype = dtype
    return c


def cfg4(dtype="bf16"):
    """BASELINE config 4 per GPU: ResNet-101 + 6/6, d_model 512, nhead 8 (800x800, batch 8)."""
    c = cfg2(dtype)
    c.backbone, c.hidden_dim = "ResNet101", 512
    return c


WORKLOADS = {"cfg2": (cfg2, 640, 16, "cfg2: ResNet-50 + 6-enc/6-dec d_model 256, 640x640"),
             "cfg4": (cfg4, 800, 8, "cfg4 (per-GPU slice): ResNet-101 + 6-enc/6-dec d_model 512 "
                                    "nhead 8, 800x800")}


def cfg5(dtype="bf16"):
    c = cfg2(dtype)
    c.dilation = True
    return c


def build(cfg, device, seed=42):
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):    # build_model's prints (caption.py:204,211)
        model, crit = build_model(cfg)
    model.load_state_dict(synthetic_state_dict(model, seed=seed))
    return model.to(device), crit


def make_optimizer(model, cfg, capturable=False, fused=False):
    """main.py:30-39: two param groups (backbone at lr_backbone), AdamW — torch's, or with
    ``fused`` the MI355X FusedAdamW (clip + AdamW in two kernels over flat arenas)."""
    groups = [{"params": [p for n, p in model.named_parameters()
                          if "backbone" not in n and p.requires_grad]},
              {"params": [p for n, p in model.named_parameters()
                          if "backbone" in n and p.requires_grad], "lr": cfg.lr_backbone}]
    if fused:
        from retr_amd.optim import FusedAdamW
        return FusedAdamW(groups, lr=cfg.lr, weight_decay=cfg.weight_decay)
    return torch.optim.AdamW(groups, lr=cfg.lr, weight_decay=cfg.weight_decay,
                             capturable=capturable)


def dump_outputs(path, loss, model):
    """--dump-outputs: what the last timed step handed its caller, as <path>/<name>.npy --
    ``loss`` (float32 [1], the step's return value) and ``param_norms`` (float64, the L2 norm of
    every trainable parameter as the step's update left it, named_parameters order).

    Both repeat from run to run of one build to about 1e-5 relative (measured: 1e-6 .. 2e-5
    after 25 steps of cfg2), which is what the default mode's atomic split-K weight-gradient
    sums allow: after one step parameters differ in the last bit only, but AdamW's normalised
    update turns a last-bit difference in a near-zero gradient into a whole +-lr step, so after
    tens of steps single parameter VALUES differ between two runs by up to ~lr (75x relative on
    small elements) and are no output two builds could be compared by; their norms are."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    params = [p.detach() for p in model.parameters() if p.requires_grad]
    norms = torch.stack([p.double().norm() for p in params])
    np.save(os.path.join(path, "loss.npy"), loss.detach().float().reshape(1).cpu().numpy())
    np.save(os.path.join(path, "param_norms.npy"), norms.cpu().numpy())
    return ["loss", "param_norms"]


def train_bench(args, rank, world, device):
    from retr_amd.engine import GraphedTrainStep, train_step
    cfg = WORKLOADS[args.workload][0]()
    model, crit = build(cfg, device)
    graphed = not args.eager
    sync = None
    if world > 1:
        from retr_amd.ddp import broadcast_parameters
        broadcast_parameters(model)
    opt = make_optimizer(model, cfg, capturable=graphed, fused=not args.torch_adamw)
    if world > 1:
        # zero-copy buckets on FusedAdamW's gradient arena; a graphed step replays its
        # forward/backward as segments cut at bucket completions and enqueues each bucket's
        # all-reduce right after the segment it completed in (overlapping the rest of backward)
        from retr_amd.ddp import GradSync
        sync = GradSync([p for p in model.parameters() if p.requires_grad],
                        bucket_mb=cfg.grad_bucket_mb, optimizer=opt)
    B, H = args.batch, args.size
    img, mask = synthetic_images(B, H, seed=1000 + rank)
    caps, cap_mask = synthetic_captions(B, cfg.max_position_embeddings, cfg.vocab_size,
                                        seed=2000 + rank)
    samples = (NestedTensor(img.to(device), mask.to(device)),)
    caps, cap_mask = caps.to(device), cap_mask.to(device)
    model.train()

    def eager_step():
        return train_step(model, crit, samples, caps, cap_mask, opt, cfg.clip_max_norm, sync)

    graph_step = GraphedTrainStep(model, crit, opt, cfg.clip_max_norm, sync) if graphed else None

    def step():
        if graph_step is not None:
            return graph_step(samples, caps, cap_mask)
        return eager_step()

    loss = None
    for _ in range(args.warmup):
        loss = step()
    if (graph_step is not None and graph_step.input_buffers() is not None
            and not args.stage_inputs):
        # the batch lives in the captured step's own input buffers (as a loader writing each
        # batch there would leave it): no per-step device-to-device staging copy
        st = graph_step.input_buffers()
        samples = (NestedTensor(st[0], st[1]),)
        caps, cap_mask = st[2], st[3]
    torch.cuda.synchronize()
    assert loss is None or torch.isfinite(loss).item(), "non-finite loss in warmup"
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    loss_v = float(loss.item())
    dumped = None
    if args.dump_outputs and rank == 0:
        # before anything below steps the model again: the state the last timed step left
        dumped = dump_outputs(args.dump_outputs, loss, model)
    if args.probe_steps <= 0:
        fam = {}
    else:
        # per-kernel HIP-event timing needs host-side launches: after the timed region, re-run
        # the identical step eagerly (same weights / inputs / stream) with the probe on
        pr = probe_mod.Probe(detail=bool(args.probe_detail))
        with pr:
            for _ in range(args.probe_steps):
                eager_step()
        torch.cuda.synchronize()
        fam = pr.summary()
    if fam and args.probe_detail and rank == 0:
        nst = max(1, args.probe_steps)
        with open(args.probe_detail, "w") as f:
            for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms_total"]):
                f.write(f"{v['ms_total'] / nst:8.3f} ms/step {v['launches'] // nst:4d}x "
                        f"{v['ms_avg'] * 1e3:8.1f} us {v['tflops']:7.1f} TF/s "
                        f"{v['gbs']:7.0f} GB/s att {v['attainable_frac']:5.3f}  {k}\n")
        fam = {}
        for k, v in pr.summary().items():
            d = fam.setdefault(k.split(" | ")[0], {"launches": 0, "ms_total": 0.0,
                                                   "flops": 0.0, "bytes": 0.0,
                                                   "attainable_ms": 0.0})
            for f in ("launches", "ms_total", "flops", "bytes", "attainable_ms"):
                d[f] += v[f]
        for d in fam.values():
            probe_mod.finish(d)
    sched = None
    if graph_step is not None and graph_step.schedule is not None:
        # the segment / bucket schedule every rank agreed on before the first replay
        sched = {"segments": len(graph_step.segments),
                 "buckets": len(graph_step.schedule["bucket_numel"]),
                 "checked_across_ranks": world}
    return dt, loss_v, fam, max(1, args.probe_steps), sched, dumped


def decode_step_bytes(cfg, B, S, T, esize):
    """Algorithmic HBM bytes of one incremental decode step at batch B: the
    decoder weights the step multiplies by (self in-proj 3C^2, out-proj C^2, cross q / out
    2C^2, FFN 2CF per layer), the MLP head (C*512 + 512^2 + 512*V), the self-attention K/V
    cache at its average length T/2 and the cross-attention K/V of the S memory tokens, all in
    the compute type (esize bytes).  cfg5 bf16, B 64: 151.6 MB."""
    C, F, L, V = cfg.hidden_dim, cfg.dim_feedforward, cfg.dec_layers, cfg.vocab_size
    weights = L * (6 * C * C + 2 * C * F) + (C * 512 + 512 * 512 + 512 * V)
    self_kv = L * 2 * C * B * (T / 2)
    cross_kv = L * 2 * C * B * S
    return esize * (weights + self_kv + cross_kv)


def decode_bench(args, rank, world, device):
    """cfg5 decode: greedy (the reference's algorithm, KV-cache incremental form) in bf16 and in
    fp32 parity mode, and beam search (beam 5; new capability), refs/sec over one batch with
    hipGraph-replayed steps."""
    from retr_amd.eval_utils.decode import IncrementalBeam, greedy
    B = args.decode_batch
    img, mask = synthetic_images(B, 224, seed=3000 + rank)
    out = {}
    for dtype in ("bf16", "fp32"):
        cfg = cfg5(dtype)
        model, _ = build(cfg, device)
        model.eval()
        samples = [NestedTensor(img.to(device), mask.to(device))]
        T = cfg.max_position_embeddings
        runs = [("greedy", lambda: greedy(samples, model, max_len=T, bos_token=101,
                                          eos_token=102))]
        if args.beam > 1 and dtype == "bf16":
            beam = IncrementalBeam(model, args.beam)
            runs.append((f"beam{args.beam}", lambda: beam(samples, T, 101, 102)))
        for name, fn in runs:
            ids = fn()                                  # warm-up (captures the step graphs)
            torch.cuda.synchronize()
            reps = []
            for _ in range(args.decode_reps):
                if world > 1:
                    dist.barrier()
                t0 = time.perf_counter()
                ids = fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if world > 1:
                    t = torch.tensor([dt], device=device)
                    dist.all_reduce(t, op=dist.ReduceOp.MAX)
                    dt = t.item()
                reps.append(dt)
            print(f"decode {name} {dtype}: " + " ".join(f"{r * 1e3:.2f}" for r in reps) + " ms",
                  file=sys.stderr, flush=True)
            dt = sorted(reps)[len(reps) // 2]           # median batch time
            out[(name, dtype)] = (dt, int((ids != 0).sum(1).max().item()))
        del model
        torch.cuda.empty_cache()
    return out


class _StopDecode(Exception):
    pass


def cpu_decode_baseline(args, cores):
    """The reference's decode algorithm (eval_utils/decode.py:53-81: one full Caption forward
    per generated token, 127 per batch) run by the CPU oracle on this host at the configured
    decode batch: k = 4 steps timed (every step is a full forward over the same [B, 128]
    caption buffer, so its cost does not depend on the step) and extrapolated x 127 / 4."""
    from oracle import model as orc
    cfg = cfg5("fp32")
    cfg.dropout = 0.0
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):
        model, _ = build_model(cfg)
    sd = synthetic_state_dict(model, seed=42)
    del model
    B, k = args.decode_batch, 4
    img, mask = synthetic_images(B, 224, seed=3000)
    T = cfg.max_position_embeddings
    times = []

    def fwd(c, m):
        if len(times) == k + 1:                 # one warm-up step + k timed steps
            raise _StopDecode
        t0 = time.perf_counter()
        lo = orc.caption_forward(sd, cfg, img, mask, c, m)
        times.append(time.perf_counter() - t0)
        return lo

    with torch.no_grad():
        try:
            orc.greedy(fwd, B, T, 101, 102)
        except _StopDecode:
            pass
    step = sum(times[1:]) / k
    per_batch = step * (T - 1)
    return {"value": round(B / per_batch, 5), "unit": "refs/s", "cores": cores, "kind": "port",
            "extrapolated": True, "seconds": round(sum(times), 2),
            "sample": f"cfg5 (R50 dilation=True 224x224, 6/6 d256), batch {B}: {k} greedy "
                      f"steps of the reference algorithm (full fp32 forward per token, "
                      f"oracle/model.py) after 1 warm-up step, {step:.3f} s/step, "
                      f"extrapolated x {T - 1}/{k} to a full batch ({per_batch:.1f} s), "
                      f"{cores} threads"}


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_threads():
    """Threads for the CPU baseline: every CPU this process may run on
    (len(os.sched_getaffinity(0))), bounded by the host's per-GPU CPU allotment when the
    launcher sets one through OMP_NUM_THREADS (the GPU box exports 16 = its CPU share for one
    GPU; using more would take cores another job was given)."""
    aff = len(os.sched_getaffinity(0))
    omp = os.environ.get("OMP_NUM_THREADS")
    return (min(aff, int(omp)) if omp and omp.isdigit() and int(omp) > 0 else aff), aff


def cpu_baseline(args, cores):
    """CPU oracle (oracle/model.py: fp32 eager torch in the reference's op order, pinned to the
    reference by tests/golden) on this host: fwd + CE + backward of the benchmarked workload at
    its configured batch, 1 warm-up step then >= 2 timed steps (more while under
    ``--cpu-seconds``), as BASELINE.md's CPU-baseline plan says."""
    from oracle import model as orc
    cfg = WORKLOADS[args.workload][0]("fp32")
    cfg.dropout = 0.0
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):
        model, _ = build_model(cfg)
    sd = synthetic_state_dict(model, seed=42)
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    del model
    sd = {k: (v.requires_grad_(True) if k in trainable else v) for k, v in sd.items()}
    B = args.cpu_batch or args.batch
    img, mask = synthetic_images(B, args.size, seed=1)
    caps, cap_mask = synthetic_captions(B, cfg.max_position_embeddings, cfg.vocab_size, seed=2)

    def step():
        for v in sd.values():
            v.grad = None
        lo = orc.caption_forward(sd, cfg, img, mask, caps[:, :-1], cap_mask[:, :-1])
        orc.caption_loss(lo, caps[:, 1:]).backward()

    step()
    n = 0
    t0 = time.perf_counter()
    while True:
        step()
        n += 1
        dt = time.perf_counter() - t0
        if (n >= 2 and dt >= args.cpu_seconds) or n >= 50:
            break
    return {"value": round(B * n / dt, 4), "unit": "images/s", "cores": cores, "kind": "port",
            "cpu": _cpu_model(), "seconds": round(dt, 2),
            "sample": f"{WORKLOADS[args.workload][3]}, batch {B}, {n} timed fwd+CE+bwd steps "
                      f"after 1 warm-up, fp32 oracle/model.py, {cores} threads"}


def _pmc_path(kind, workload):
    """The committed rocprofv3 --pmc summary of ``kind`` ("traffic" / "mfma") for ``workload``:
    profiles/pmc_<kind>_<workload>.json.  Counters are only ever reported for the workload they
    were collected on: no file, no counter fields."""
    return os.path.join(ROOT, "profiles", f"pmc_{kind}_{workload}.json")


def _traffic(family, workload):
    """Per-launch HBM bytes of ``family`` from the workload's committed rocprofv3 --pmc pass
    (profiles/pmc_traffic_<workload>.json, written by tools/pmc_traffic.py with the gfx950
    FETCH_SIZE x2 correction), or None when no counter pass covers it."""
    path = _pmc_path("traffic", workload)
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        return None, None
    ent = d.get("families", {}).get(family)
    if not ent:
        return None, None
    return ent, d.get("source")


def _traffic_fields(family, calls_per_step, bytes_per_call, workload):
    """Counted HBM traffic of ``family`` in both units: per kernel DISPATCH (what the --pmc pass
    measures) and per retr_* API CALL (what the probe times; one call can dispatch several
    kernels), with the counted / algorithmic ratio per call."""
    ent, src = _traffic(family, workload)
    if not ent:
        return {"traffic": None, "traffic_source": None}
    out = {"traffic": ent.get("bytes_per_launch"), "traffic_unit": "bytes per dispatch",
           "traffic_source": src}
    dps = ent.get("dispatches_per_step")
    if dps and calls_per_step:
        per_call = ent["bytes_per_launch"] * dps / calls_per_step
        out.update({"dispatches_per_step": round(dps, 2),
                    "traffic_per_call": round(per_call),
                    "traffic_over_algorithmic": round(per_call / bytes_per_call, 3)
                    if bytes_per_call else None})
    return out


def _roofline(fam, psteps, workload):
    """Roofline object of the dominant kernel family (most device time per step).  Its bound is
    set by its arithmetic intensity (algorithmic FLOP / algorithmic HBM bytes, summed over its
    launches) against the ridge point 2.5 PF / 8 TB/s = 312.5 FLOP/B: below it the family is
    HBM-bound and achieved / peak are GB/s, above it TFLOP/s.  ``attainable_frac`` is the
    sharper figure for a family that mixes both kinds of launch: sum over launches of
    max(FLOP / 2.5 PF, bytes / 8 TB/s) over the measured time."""
    dom_key = max(fam, key=lambda k: fam[k]["ms_total"]) if fam else None
    if dom_key is None:
        return None
    d = fam[dom_key]
    hbm = d["intensity"] < probe_mod.RIDGE
    if hbm:
        achieved, peak, unit = d["gbs"], PEAK_HBM_GBS, "GB/s"
    else:
        achieved, peak, unit = d["tflops"], PEAK_BF16_TFLOPS, "TFLOP/s"
    n = max(1, d["launches"])
    tf = _traffic_fields(dom_key, d["launches"] / psteps, d["bytes"] / n, workload)
    return {"bound": "hbm" if hbm else "mfma", "kernel": dom_key,
            "kernel_symbol": probe_mod.FAMILY_SYMBOL.get(dom_key, dom_key),
            "achieved": round(achieved, 2), "peak": peak, "unit": unit,
            "frac": round(achieved / peak, 4), **tf,
            "intensity_flop_per_byte": round(d["intensity"], 1),
            "ridge_flop_per_byte": probe_mod.RIDGE,
            "tflops": round(d["tflops"], 2), "mfma_frac": round(d["tflops"] / PEAK_BF16_TFLOPS, 4),
            "gbs": round(d["gbs"], 1), "hbm_frac": round(d["gbs"] / PEAK_HBM_GBS, 4),
            "attainable_frac": round(d["attainable_frac"], 4),
            "mfma_busy": _mfma_busy(dom_key, workload),
            "api_calls_per_step": d["launches"] // psteps,
            "avg_launch_us": round(d["ms_avg"] * 1e3, 2),
            "flops_per_launch": round(d["flops"] / n, 1),
            "bytes_per_launch": round(d["bytes"] / n),
            "launch_unit": "one retr_* API call (may dispatch several kernels: dispatches_per_step)",
            "timing": "HIP events around each launch on torch's current stream (the stream "
                      "every retr kernel runs on), device spin in front so the events bracket "
                      "device time only; eager re-run of the step"}


def _mfma_busy(family, workload):
    """MFMA-busy fraction of ``family`` from the workload's committed rocprofv3 --pmc pass
    (profiles/pmc_mfma_<workload>.json, tools/pmc_mfma.py): SQ_VALU_MFMA_BUSY_CYCLES over
    (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs), i.e. rocprof's MfmaUtil per launch."""
    try:
        with open(_pmc_path("mfma", workload)) as f:
            d = json.load(f)
    except (OSError, ValueError):
        return None
    ent = d.get("families", {}).get(family)
    return None if not ent else ent.get("mfma_busy")


def init_dist(local, backend="nccl"):
    """One process per GPU from the torchrun environment (RANK / WORLD_SIZE / MASTER_*), RCCL
    ("nccl") over xGMI, with the bench's short collective timeout (DIST_TIMEOUT)."""
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if backend == "nccl":
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local),
                                timeout=DIST_TIMEOUT)
    else:
        dist.init_process_group(backend, timeout=DIST_TIMEOUT)


def parse_args(argv=None):
    """The command line.  Without ``--full`` the run is the plain one: the probe, the decode
    block and the CPU baselines are off, and asking for one of them is an error."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the per-kernel probe "
                         "and roofline, the cfg5 decode block and the CPU baselines")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the last timed step's loss and the L2 norm of every parameter "
                         "it updated as DIR/<name>.npy")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cfg2",
                    help="cfg2 (default, BASELINE metric) or cfg4's per-GPU slice")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (0: the workload's)")
    ap.add_argument("--size", type=int, default=0, help="image side (0: the workload's)")
    ap.add_argument("--decode-batch", type=int, default=64)
    ap.add_argument("--beam", type=int, default=5, help="beam width of the decode block (1: off)")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--decode-reps", type=int, default=3,
                    help="timed decode batches per mode (median reported)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=8.0,
                    help="CPU-baseline sample: timed oracle steps (>= 2) until this much time")
    ap.add_argument("--cpu-batch", type=int, default=0, help="CPU-baseline batch (0: --batch)")
    ap.add_argument("--eager", action="store_true", help="no hipGraph capture of the step")
    ap.add_argument("--probe-steps", type=int, default=None,
                    help="eager steps re-run under the per-kernel probe (--full; default 2)")
    ap.add_argument("--torch-adamw", action="store_true",
                    help="torch.optim.AdamW(capturable) + clip_grad_norm_ instead of the default "
                         "retr_amd FusedAdamW (clip + AdamW kernels over flat arenas)")
    ap.add_argument("--probe-detail", default="", help="write a per-shape kernel table here")
    ap.add_argument("--stage-inputs", action="store_true",
                    help="copy the batch into the captured step's input buffers every step "
                         "(the pre-round-4 timing; default: the batch already sits there)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if not args.full:
        if args.probe_detail or (args.probe_steps or 0) > 0:
            ap.error("--probe-detail / --probe-steps need --full (the probe runs only there)")
        args.probe_steps, args.no_decode, args.no_cpu_baseline = 0, True, True
    elif args.probe_steps is None:
        args.probe_steps = 2
    _, size, batch, _ = WORKLOADS[args.workload]
    args.size = args.size or size
    args.batch = args.batch or batch
    if args.workload != "cfg2":
        args.no_decode = True                  # the decode block is config 5's
    return args


def main():
    args = parse_args()
    wl_desc = WORKLOADS[args.workload][3]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        init_dist(local)
    device = torch.device("cuda", local)
    torch.manual_seed(42 + rank)

    dt, loss, fam, psteps, sched, dumped = train_bench(args, rank, world, device)
    imgs = world * args.batch * args.steps
    value = imgs / dt
    roof = _roofline(fam, psteps, args.workload)
    families = {k: {"ms_per_step": round(v["ms_total"] / psteps, 3),
                    "tflops": round(v["tflops"], 1), "gbs": round(v["gbs"], 1),
                    "bound": "hbm" if v["intensity"] < probe_mod.RIDGE else "mfma",
                    "attainable_frac": round(v["attainable_frac"], 4),
                    "api_calls_per_step": v["launches"] // psteps,
                    **{f: t for f, t in _traffic_fields(
                        k, v["launches"] / psteps, v["bytes"] / max(1, v["launches"]),
                        args.workload).items()
                       if f in ("dispatches_per_step", "traffic", "traffic_per_call",
                                "traffic_over_algorithmic")}}
                for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms_total"])}
    cores, aff = cpu_threads()
    decode = None
    if not args.no_decode:
        res = decode_bench(args, rank, world, device)
        cfg = cfg5()
        S, T = 14 * 14, cfg.max_position_embeddings
        decode = {"metric": "greedy-decode refs/sec"}
        for dtype, esz in (("bf16", 2), ("fp32", 4)):
            ddt, steps = res[("greedy", dtype)]
            by = decode_step_bytes(cfg, args.decode_batch, S, T, esz)
            nsteps = T - 1
            ent = {"value": round(world * args.decode_batch / ddt, 2), "unit": "refs/s",
                   "batch_per_gpu": args.decode_batch, "steps": nsteps,
                   "ms_per_batch": round(ddt * 1e3, 2),
                   "bytes_per_step": round(by),
                   "hbm_frac": round(by * nsteps / ddt / (PEAK_HBM_GBS * 1e9), 4),
                   "hbm_frac_basis": "algorithmic bytes per step x 127 steps / whole batch "
                                     "time (encode included) / 8 TB/s"}
            if dtype == "bf16":
                ent["config"] = ("cfg5: ResNet-50 dilation=True 224x224, 6/6 d256, bf16 "
                                 "operands, KV-cache greedy, per-step hipGraphs; ids are NOT "
                                 "guaranteed equal to the reference's (bf16 rounding flips "
                                 "near-tie argmaxes; tests/test_gpu_configs.py)")
            else:
                ent["config"] = ("cfg5 in fp32 parity mode (every value fp32; the step as "
                                 "three fused launches per decoder layer, csrc/decode_f32.hip, "
                                 "exact-f32 MFMA / FMA chains): token ids equal to the reference "
                                 "algorithm (tests/test_gpu_configs.py: B=64 vs the "
                                 "full-recompute algorithm, B=2 and 4 rows of B=64 vs the CPU "
                                 "oracle)")
            decode[dtype] = ent
        decode["value"] = decode["bf16"]["value"]
        decode["unit"] = "refs/s"
        for (name, dtype), (bdt, bsteps) in res.items():
            if name != "greedy":
                decode[name] = {"value": round(world * args.decode_batch / bdt, 2),
                                "unit": "refs/s", "ms_per_batch": round(bdt * 1e3, 2),
                                "dtype": dtype}
        if rank == 0 and world == 1 and not args.no_cpu_baseline:
            torch.set_num_threads(cores)
            decode["cpu_baseline"] = cpu_decode_baseline(args, cores)
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        torch.set_num_threads(cores)
        cpu = cpu_baseline(args, cores)
        cpu["affinity_cpus"] = aff
    if rank == 0:
        if world == 1:
            launch = "eager" if args.eager else "hipGraph (whole step)"
        else:
            launch = ("eager, per-bucket RCCL all-reduce from post-accumulate-grad hooks"
                      if args.eager else
                      "hipGraph segments of fwd+bwd cut at gradient-bucket completions, each "
                      "bucket's RCCL all-reduce (AVG, in place on the gradient arena) enqueued "
                      "after its segment and overlapping the next ones, then hipGraph "
                      "(clip+AdamW) after all buckets")
        out = {"metric": METRIC, "value": round(value, 2), "unit": "images/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "full": args.full,
               "outputs_dumped": dumped,
               "data": "synthetic (RefCOCO-shaped images/captions, synthetic weights)",
               "config": {"workload": f"{wl_desc}, batch {args.batch}/GPU, "
                                      "fwd+CE+bwd+allreduce+clip+AdamW",
                          "global_batch": world * args.batch, "seq_len": 128,
                          "parallelism": f"dp{world}"},
               "loss": round(loss, 4), "roofline": roof, "cpu_baseline": cpu,
               "launch": launch,
               "dist": {"world_size_seen": dist.get_world_size() if dist.is_initialized() else 1,
                        "backend": dist.get_backend() if dist.is_initialized() else None,
                        "dp_schedule": sched},
               "optimizer": "torch.optim.AdamW" if args.torch_adamw else "FusedAdamW",
               "input_staging": ("per-step device-to-device copy into the captured step's "
                                 "input buffers (--stage-inputs)" if args.stage_inputs or
                                 args.eager else
                                 "none: the batch is resident in the captured step's input "
                                 "buffers, as a loader writing each batch there leaves it "
                                 "(since round 4; rounds 1-3 timed a 78.6 MB staging copy "
                                 "per step, ~45 us)"),
               "decode": decode, "kernel_families": families}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
