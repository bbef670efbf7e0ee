"""Teacher-forced scoring of given expressions: per-token and per-expression log-likelihoods
(how referring-expression models are reranked, and what a perplexity is computed from)."""
import torch

_MASKED = -100      # stands for a masked position in the targets; never a class id


@torch.no_grad()
def score_expressions(samples, model, caps, cap_masks):
    """Log-likelihood of the expressions ``caps`` [B, T+1] (bos first) under ``model``.

    ``samples`` are the model's encoder inputs as for ``greedy`` (a sequence, passed as
    ``model(*samples, ...)``); ``cap_masks`` [B, T+1] is True at padded positions.  One forward on
    ``caps[:, :-1]`` in eval mode, then the cross-entropy kernel with ``reduction='none'`` and the
    positions where ``cap_masks[:, 1:]`` is True as the ignored set (they score 0).

    Returns ``(token_logprob [B, T], seq_logprob [B], n_tokens [B])``: log p(caps[b, t+1] | caps[b,
    :t+1], image), their sum over the unmasked positions, and the number of those positions.
    """
    from .. import ops
    was_training = model.training
    model.eval()
    try:
        dev = caps.device
        samples = [s.to(dev) for s in samples]
        logits = model(*samples, caps[:, :-1], cap_masks[:, :-1])
    finally:
        model.train(was_training)
    masked = cap_masks[:, 1:]
    target = caps[:, 1:].masked_fill(masked, _MASKED)
    nll = ops.cross_entropy(logits.permute(0, 2, 1), target, ignore_index=_MASKED,
                            reduction="none")
    token_logprob = 0.0 - nll
    return token_logprob, token_logprob.sum(1), (~masked).sum(1)
