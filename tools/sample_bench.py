"""What sampling costs over greedy's select step: greedy against
``sample(temperature=0.7, top_p=0.9)`` in one process at the cfg5 decode shape (R50 dilated
224^2, 6/6 d256, V 30522, T 128, batch 64, bf16), refs/s = batch / median of 3 batches after
one warm batch (which captures the step graphs).  The EOS id is one that never occurs, so both
decoders run all 127 steps.  Informational: it gates nothing.

    python tools/sample_bench.py [--out profiles/sampling_decode.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import build, cfg5  # noqa: E402
from retr_amd.eval_utils.decode import IncrementalSampler, greedy  # noqa: E402
from retr_amd.models.utils import NestedTensor  # noqa: E402
from retr_amd.synthetic import synthetic_images  # noqa: E402


def batch_times(fn, reps):
    fn()                                            # warm batch
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_decode.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench: needs the GPU (a CPU run measures nothing)")
    dev = "cuda"
    cfg = cfg5("bf16")
    model, _ = build(cfg, dev)
    model.eval()
    T, B = cfg.max_position_embeddings, args.batch
    img, mask = synthetic_images(B, 224, seed=3000)
    samples = [NestedTensor(img.to(dev), mask.to(dev))]
    sampler = IncrementalSampler(model, temperature=0.7, top_p=0.9, seed=1)
    runs = [("greedy", lambda: greedy(samples, model, max_len=T, bos_token=101, eos_token=-1)),
            ("sample(temperature=0.7, top_p=0.9)", lambda: sampler(samples, T, 101, -1))]
    lines = [f"cfg5 decode, bf16, batch {B}, T {T}, V {cfg.vocab_size}, {T - 1} steps per batch "
             f"(EOS never occurs), {torch.cuda.get_device_properties(0).gcnArchName}",
             f"refs/s = batch / median of {args.reps} batches after one warm batch"]
    rate = {}
    for name, fn in runs:
        ts = batch_times(fn, args.reps)
        med = sorted(ts)[len(ts) // 2]
        rate[name] = B / med
        lines.append(f"{name}: {B / med:.1f} refs/s  (median {med * 1e3:.2f} ms/batch; batches "
                     + " ".join(f"{t * 1e3:.2f}" for t in ts) + " ms)")
    g, s = (rate[n] for n, _ in runs)
    lines.append(f"sampling / greedy: {s / g:.3f}  (+{(B / s - B / g) / (T - 1) * 1e6:.1f} us "
                 f"per step for the draw in place of the argmax)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
