"""CPU-side checks of the cross-entropy options: what Config / build_model construct, and the
refusals that stay (class weights, CPU tensors)."""
import pytest
import torch

from retr_amd.models.caption import CrossEntropyLoss, build_model
from tests.helpers import make_config


def test_config_defaults_give_the_reference_criterion():
    c = make_config()
    assert c.label_smoothing == 0.0 and c.loss_ignore_pad is False
    _, crit = build_model(c)
    assert isinstance(crit, CrossEntropyLoss)
    assert crit.ignore_index == -100 and crit.label_smoothing == 0.0
    assert crit.reduction == "mean" and crit.weight is None


def test_config_options_reach_the_criterion():
    c = make_config()
    c.loss_ignore_pad, c.label_smoothing = True, 0.1
    c.pad_token_id = 7
    _, crit = build_model(c)
    assert crit.ignore_index == c.pad_token_id == 7
    assert crit.label_smoothing == 0.1 and crit.reduction == "mean"


def test_class_weights_stay_unsupported():
    crit = CrossEntropyLoss(weight=torch.ones(11), ignore_index=0)
    with pytest.raises(NotImplementedError):
        crit(torch.zeros(2, 11, 3), torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(NotImplementedError):       # logits must be [B, V, T]
        CrossEntropyLoss(ignore_index=0)(torch.zeros(6, 11), torch.zeros(6, dtype=torch.long))


@pytest.mark.parametrize("kw", [{}, {"ignore_index": 0}, {"label_smoothing": 0.1},
                                {"reduction": "sum"}, {"reduction": "none"}])
def test_no_cpu_fallback(kw):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CrossEntropyLoss(**kw)(torch.zeros(2, 11, 3), torch.zeros(2, 3, dtype=torch.long))


def test_invalid_options_raise():
    from retr_amd import ops
    x, t = torch.zeros(2, 11, 3), torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ValueError):
        ops.cross_entropy(x, t, reduction="batchmean")
    with pytest.raises(ValueError):
        ops.cross_entropy(x, t, label_smoothing=1.5)
