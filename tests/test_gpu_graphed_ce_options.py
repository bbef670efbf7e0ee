"""The captured training step (engine.GraphedTrainStep) with the cross-entropy options: the
mean's denominator follows the batch that is replayed.

Kept apart from test_gpu_ce_options.py so that it runs after test_gpu_ddp.py.  GraphedTrainStep
takes a stream from torch's 32-slot round-robin pool, and the process group of test_gpu_ddp.py
takes its RCCL stream from the same pool: were the tests before test_gpu_ddp.py to take two more
pool streams than they do (31), the RCCL stream would be the very stream torch.cuda.graph captures
on by default, and the watchdog's event query during the single-graph capture of
test_segmented_dp_step_cfg2_equals_single_graph_bitwise aborts the process
(hipErrorCapturedEvent).  test_gpu_ce_options.py therefore takes no pool stream of its own."""
import pytest
import torch

from retr_amd import _lib
from retr_amd.models.caption import build_model
from retr_amd.models.utils import NestedTensor
from retr_amd.synthetic import synthetic_captions, synthetic_images, synthetic_state_dict
from tests.helpers import make_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
OLD_CALLS = {"retr_ce_fwd", "retr_ce_bwd", "retr_ce_fwd_bwd", "retr_ce_bwd_rescale"}


class _Recorder:
    """Stand-in for retr_amd.probe.Probe: records the name of every library call."""

    def __init__(self):
        self.names = set(_lib.exported_symbols())
        self.called = []

    def wrap(self, name, args, fn):
        self.called.append(name)
        return fn()


def test_graphed_train_step_follows_the_batch_pad_count():
    """engine.GraphedTrainStep with the criterion Config builds for loss_ignore_pad +
    label_smoothing (bf16: the one-pass kernel inside the capture), replayed on batches whose
    captions have different lengths, against the same steps run eagerly.  The bar is
    test_graphed_bf16_step_matches_eager_then_eval's for this comparison (2e-3 on the loss); a
    denominator fixed at capture time would be off by the ratio of the pad counts."""
    from retr_amd.engine import GraphedTrainStep, train_step
    from retr_amd.optim import FusedAdamW

    def make():
        cfg = make_config(dtype="bf16")
        cfg.loss_ignore_pad, cfg.label_smoothing = True, 0.1
        model, crit = build_model(cfg)
        model.load_state_dict(synthetic_state_dict(model, seed=42))
        model.to(DEV).train()
        groups = [{"params": [p for n, p in model.named_parameters()
                              if "backbone" not in n and p.requires_grad]},
                  {"params": [p for n, p in model.named_parameters()
                              if "backbone" in n and p.requires_grad], "lr": cfg.lr_backbone}]
        return cfg, model, crit, FusedAdamW(groups, lr=cfg.lr, weight_decay=cfg.weight_decay)

    cfg, m1, crit, o1 = make()
    _, m2, _, o2 = make()
    assert crit.ignore_index == cfg.pad_token_id == 0 and crit.label_smoothing == 0.1
    img, mask = synthetic_images(2, 64, seed=5)
    samples = (NestedTensor(img.to(DEV), mask.to(DEV)),)
    graphed = GraphedTrainStep(m1, crit, o1, 0.1, warmup=2)
    rec = _Recorder()
    counts = set()
    for seed in (6, 7, 8):
        caps, cm = synthetic_captions(2, cfg.max_position_embeddings, cfg.vocab_size, seed=seed)
        counts.add(int((caps[:, 1:] != 0).sum()))
        caps, cm = caps.to(DEV), cm.to(DEV)
        lg = graphed(samples, caps, cm).item()
        _lib.set_probe(rec)
        try:
            le = train_step(m2, crit, samples, caps, cm, o2, 0.1).item()
        finally:
            _lib.set_probe(None)
        assert abs(lg - le) <= 2e-3 * abs(le), (seed, lg, le)
    assert len(counts) > 1, counts
    assert {"retr_ce_count", "retr_ce_fwd_bwd_opt"} <= set(rec.called)
    assert not OLD_CALLS & set(rec.called)
