"""``MultiChannelAE`` (reference networks/acai_multi_channel.py:22-103): the auto-encoder that super-resolves a label map together
with its image.  Input = two channels (intensity, class id), one shared latent, a decoder trunk that ends in ``depth`` feature maps and
two heads on it: ``decoder_head1`` -> sigmoid image, ``decoder_head2`` -> softmax class probabilities.

Same constructor arguments, state_dict keys, ``named_parameters()`` order and initialisation (same draws from the same generator) as
the reference; the modules are parameter holders and every pass runs on the HIP engine: ``enc``, ``dec``, ``decoder_head1`` and
``decoder_head2`` WITHOUT its Softmax are four compiled stacks (``HipAE._runner``), the softmax / soft-Dice / arg-max of the label head is
``ops.softmax_dice`` (csrc/seg_head.hip), and torch autograd adds the two heads' gradients at the trunk output."""
import torch
import torch.nn as nn

from .. import _hip, engine, ops
from .acai_vanilla import HipAE, Initializer, _block, activation, num_scales  # noqa: F401
from .acai_vanilla_modified import Encoder  # noqa: F401  (LargerAE's: depth // 2 stem)

STACKS = ("enc", "dec", "decoder_head1", "decoder_head2")


def Decoder(scales, depth, latent, colors, n_res_block=None, use_upsample=True, use_batchnorm=False):
    """reference :44-64: LargerAE's decoder trunk -- 1x1 conv + LeakyReLU (+ BatchNorm), the blocks, conv3x3(kp -> depth) + LeakyReLU;
    no output convolution and no sigmoid (the heads follow).  ``colors`` is accepted and unused, as in the reference."""
    if n_res_block is not None or not use_upsample:
        raise NotImplementedError("ResBlock / ConvTranspose decoders are not part of this build")
    c1 = depth << scales
    layers = [nn.Conv2d(latent, c1, 1, padding=0), activation()]
    if use_batchnorm:
        layers.append(nn.BatchNorm2d(c1))
    kp = c1
    for scale in range(scales - 1, -1, -1):
        k = depth << scale
        layers += _block(kp, k, use_batchnorm)
        layers.append(nn.Upsample(scale_factor=2))
        kp = k
    layers += [nn.Conv2d(kp, depth, 3, padding=1), activation()]
    Initializer(layers)
    return nn.Sequential(*layers)


class MultiChannelAE(HipAE):

    def __init__(self, args):
        super().__init__()
        scales = num_scales(args)
        self._fill_defaults(args)
        depth, nclasses = int(args["depth"]), int(args["nclasses"])
        if nclasses % 4 != 0 or not _hip.SEG_MIN_CLASSES <= nclasses <= _hip.SEG_MAX_CLASSES:
            raise ValueError("MultiChannelAE: nclasses=%d is not supported -- the 1x1 classifier runs on the matrix-core convolution, whose "
                             "channel counts are multiples of 4, and the label head takes %d to %d classes: use nclasses 4 or 8"
                             % (nclasses, _hip.SEG_MIN_CLASSES, _hip.SEG_MAX_CLASSES))
        self.nclasses = nclasses
        self.enc = Encoder(scales, depth, args["latent"], args["colors"], n_res_block=args["n_res_block"],
                           use_batchnorm=args["use_batchnorm"]).to(args["device"])
        self.dec = Decoder(scales, depth, args["latent"], args["colors"], n_res_block=args["n_res_block"],
                           use_batchnorm=args["use_batchnorm"]).to(args["device"])
        # reference :85-91: both heads are BUILT, then both initialised (the order of the draws from the generator)
        head1 = [nn.Conv2d(depth, 1, 3, padding=1), nn.Sigmoid()]
        head2 = [nn.Conv2d(depth, depth, 3, padding=1), activation(), nn.BatchNorm2d(depth), nn.Conv2d(depth, nclasses, 1, padding=0),
                 nn.Softmax(dim=1)]
        Initializer(head1)
        Initializer(head2)
        self.decoder_head1 = nn.Sequential(*head1)
        self.decoder_head2 = nn.Sequential(*head2)

    # ---- the four stacks -----------------------------------------------------------------------------------------------------------
    def _runner(self, name):
        cache = self.__dict__.setdefault("_runners", {})
        r = cache.get(name)
        if r is None:
            seq = getattr(self, name)
            if name == "decoder_head2":
                seq = nn.Sequential(*list(seq)[:-1])          # the logits: the Softmax belongs to ops.softmax_dice (not registered anywhere)
            r = cache[name] = engine.SequentialRunner(seq)
        return r

    def prepare_weights(self, names=STACKS):
        super().prepare_weights(names)

    def ensure_bn_barriers(self, names=STACKS):
        super().ensure_bn_barriers(names)

    def set_sync_bn(self, fn, count_scale=1.0, p2p=None):
        raise NotImplementedError("MultiChannelAE is single-process: data parallel is not built for the multi-channel trainers")

    def max_elems_per_image(self, what, chw):
        C, H, W = (int(v) for v in chw)
        if what == "encode":
            return self._runner("enc").trace_shapes(H, W, C)[0]
        if what == "forward":
            e, (H, W, C) = self._runner("enc").trace_shapes(H, W, C)
        elif what == "decode":
            e = 0
        else:
            return None
        d, (h, w, c) = self._runner("dec").trace_shapes(H, W, C)
        return max(e, d, self._runner("decoder_head1").trace_shapes(h, w, c)[0], self._runner("decoder_head2").trace_shapes(h, w, c)[0])

    # ---- passes ----------------------------------------------------------------------------------------------------------------------
    def _heads(self, trunk, splits, needs_grad):
        """trunk: ONE logical-NCHW tensor [sum(splits), depth, H, W] -> per sub-batch {'image' NCHW, 'logits' NHWC}; each sub-batch keeps
        its own BatchNorm statistics in ``decoder_head2``, in order."""
        t = engine.to_nhwc(trunk)
        images = self._pass_batched("decoder_head1", t, splits, needs_grad)
        logits = self._pass_batched("decoder_head2", t, splits, needs_grad)
        return [{"image": im, "logits": engine.to_nhwc(lg)} for im, lg in zip(images, logits)]

    def decode_multi(self, latents, needs_grad=None):
        """``HipAE.decode_multi`` for the two-headed decoder: one launch sequence per stack for all sub-batches, BatchNorm statistics per
        sub-batch in the order given (the reference's ``dec(z)`` then ``dec(z_mix)``).  Returns one {'image', 'logits'} per sub-batch;
        the probabilities come from ``ops.softmax_dice`` (with the loss) or ``ops.softmax_argmax``."""
        needs_grad = [True] * len(latents) if needs_grad is None else list(needs_grad)
        if any(g and not p for p, g in zip(needs_grad[:-1], needs_grad[1:])):
            raise ValueError("sub-batches that need gradients must come first")
        zs = [engine.to_nhwc(z) for z in latents]
        splits = [z.shape[0] for z in zs]
        x = zs[0] if len(zs) == 1 else torch.cat(zs, dim=0)
        trunk = self._pass_batched("dec", x, splits, needs_grad, merge=True)[0]
        return self._heads(trunk, splits, needs_grad)

    def decode_logits(self, z):
        return self.decode_multi([z])[0]

    def decode(self, z):
        out = self.decode_logits(z)
        return {"image": out["image"], "soft_probs": engine.to_nchw_view(ops.softmax_nhwc(out["logits"]))}

    def decode_labels(self, z):
        """Inference: {'image', 'soft_probs', 'pred_labels' int64 [N, 1, H, W]} with the arg-max taken in the softmax pass."""
        with torch.no_grad():
            out = self.decode_logits(z)
            probs, amax = ops.softmax_argmax(out["logits"])
        return {"image": out["image"], "soft_probs": engine.to_nchw_view(probs), "pred_labels": amax.unsqueeze(1).long()}

    def decode_mixes(self, z, alphas):
        """``HipAE.decode_mixes`` for the two-headed decoder: the in-between slices AND label maps of a whole volume from the same mixed
        latents.  Returns {'image' [n (Z - 1), 1, H, W], 'soft_probs', 'pred_labels'} (row k (Z - 1) + i), or None as the base does."""
        trunk = super().decode_mixes(z, alphas)
        if trunk is None:
            return None
        with torch.no_grad():
            out = self._heads(trunk, [trunk.shape[0]], [False])[0]
            probs, amax = ops.softmax_argmax(out["logits"])
        return {"image": out["image"], "soft_probs": engine.to_nchw_view(probs), "pred_labels": amax.unsqueeze(1).long()}

    def decode_mixes_at(self, z, gap_alphas):
        """``HipAE.decode_mixes_at`` for the two-headed decoder: {'image' [S, 1, H, W], 'soft_probs', 'pred_labels'} for the S mixes,
        gap-major in ascending position, or None as the base does."""
        trunk = super().decode_mixes_at(z, gap_alphas)
        if trunk is None:
            return None
        with torch.no_grad():
            out = self._heads(trunk, [trunk.shape[0]], [False])[0]
            probs, amax = ops.softmax_argmax(out["logits"])
        return {"image": out["image"], "soft_probs": engine.to_nchw_view(probs), "pred_labels": amax.unsqueeze(1).long()}

    def forward(self, img):
        return self.decode(self.encode(img))
