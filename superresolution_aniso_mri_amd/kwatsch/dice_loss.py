"""Soft-Dice loss of the label head with the reference's signatures (kwatsch/dice_loss.py:4-33).

``soft_dice_score`` / ``DiceLoss.forward`` take SOFT PROBABILITIES [N, K, H, W], as the reference does, and are written in tensor
operations: they serve callers that already hold probabilities (validation of stored predictions, host-side checks) and run on any
device.  The training step does not come through here: the trainers differentiate ``ops.softmax_dice``, which goes from the logits to
the loss in one kernel pass (csrc/seg_head.hip); ``DiceLoss.from_logits`` is that path.

Deviation: a target outside [0, n_classes) belongs to no class here, where the reference's ``scatter_`` raises."""
import torch


def soft_dice_score(prob_c, one_hot):
    """-mean over (sample, class) of 2 sum(one_hot * p) / (sum(one_hot) + sum(p) + 1e-6), sums over the two image dimensions."""
    eps = 1.0e-6
    nominator = 2 * torch.sum(one_hot * prob_c, dim=(2, 3))
    denominator = torch.sum(one_hot, dim=(2, 3)) + torch.sum(prob_c, dim=(2, 3)) + eps
    return -torch.mean(nominator / denominator)


class DiceLoss(torch.nn.Module):

    def __init__(self, n_classes):
        super(DiceLoss, self).__init__()
        self.n_classes = n_classes

    def forward(self, input, target):
        """input: soft probabilities [N, K, H, W]; target: class ids [N, H, W] (any integer or float type)."""
        classes = torch.arange(input.shape[1], device=input.device, dtype=torch.float32).view(1, -1, 1, 1)
        one_hot = (target.unsqueeze(1).to(torch.float32) == classes).to(input.dtype)
        return soft_dice_score(input, one_hot)

    def from_logits(self, logits_nhwc, target, want_argmax=False):
        """The fused device path: (loss, probs NHWC, argmax or None) of ``ops.softmax_dice``."""
        from .. import ops
        if logits_nhwc.shape[-1] != self.n_classes:
            raise ValueError("DiceLoss(%d) got logits with %d classes" % (self.n_classes, logits_nhwc.shape[-1]))
        return ops.softmax_dice(logits_nhwc, target, want_argmax=want_argmax)
