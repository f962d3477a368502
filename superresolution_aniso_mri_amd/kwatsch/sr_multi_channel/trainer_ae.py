"""``MultiChannelTrainer`` / ``MultiChannelCAISRTrainer``: the trainers of the two-channel (image, label map) auto-encoder of the reference
(kwatsch/sr_multi_channel/trainer_ae.py:66-424) on the HIP engine -- rows ("ae", "ACDCLBL") and ("ae_combined", "ACDCLBL") of
networks/net_config.py, model ``networks/acai_multi_channel.py``.

Per step, x = batch['image'] [2B, 2, H, W] (channel 0 intensity, channel 1 class id), between = batch['slice_between'] [B, 2, H, W]:
    z = enc(x);  (image, soft_probs) = heads(dec(z))
    loss_ae    = MSE(x[:, :1], image)                          (get_loss: LPIPS with --use_percept_loss, + LapLoss)
    loss_label = 0.1 * Dice(soft_probs, x[:, 1])
    loss_latent_1 = MSE(0.5 z[:B] + 0.5 z[B:], enc(between))   logged only; ``between`` is encoded in EVAL mode under no_grad
                                                               (get_latent_loss(no_grad=True)): no BatchNorm update, unlike AETrainerEndToEnd
  MultiChannelTrainer:       loss = loss_ae + loss_label.  The 0.5 mix is decoded AFTER the optimizer step, in eval mode, for the logged
                             predictions, and the model is LEFT in eval mode: every BatchNorm layer is updated once per step.
  MultiChannelCAISRTrainer:  (s_mix, p_mix) = heads(dec(z_mix)) in TRAIN mode; loss = loss_ae + loss_label + w * (image loss(between[:, :1],
                             s_mix) + Dice(p_mix, between[:, 1])), w = ex_loss_weight1 or the annealing table.  dec(z) and dec(z_mix)
                             run as ONE launch sequence per stack with two BatchNorm statistic groups in that order: the encoder's layers
                             are updated once, the decoder's and the label head's twice; the model is left in train mode.
The Dice terms go from the LOGITS to the loss in one kernel pass and back in one (``ops.softmax_dice``, csrc/seg_head.hip), reading
the labels in place from channel 1 of the batch.

``train()`` is a thin wrapper around ``_step_core`` (device-resident inputs, no host read of a device value), so that
``enable_step_graph`` replays the step from one HIP graph launch for launch (``AEBaseTrainer._train_graphed``): steps that keep their
predictions and eval steps stay eager, and the eval-mode encoder pass inside the step gets its BatchNorm scale / shift from a launch of
the graph.  ``validate(image_dict=...)`` previews whole held-out volumes -- images AND label maps -- and scores the synthesised label
maps on the device beside the nearest-slice baseline (``_generate_val_volumes``).  Single process (data parallel raises, as
``ACAITrainer`` does); the reference's CPU round-trip chunking is not reproduced (eval-mode BatchNorm makes chunked == unchunked)."""
import os

import numpy as np
import torch

from ... import ops
from ..acai_utils import make_grid, save_image_grid
from ..cardiac.trainer_ae import CombinedStepMixin
from ..dice_loss import DiceLoss
from ..trainer_ae import AEBaseTrainer

LABEL_WEIGHT = 0.1      # reference :94


def generate_recon_grid(img_ref, label_ref, img_recons, pred_labels, nclasses=3, max_items=16):
    """reference :12-33: (image grid, label grid), rows = reference / prediction / difference; labels divided by ``nclasses``."""
    img_ref, label_ref = img_ref.detach().cpu().float(), label_ref.detach().cpu().float()
    img_recons, pred_labels = img_recons.detach().cpu().float(), pred_labels.detach().cpu().float()
    k = min(max_items, img_recons.size(0))
    recons = torch.cat([img_ref[:k], img_recons[:k], img_ref[:k] - img_recons[:k]], dim=0)
    labels = torch.cat([label_ref[:k], pred_labels[:k], label_ref[:k] - pred_labels[:k]], dim=0) / nclasses
    return make_grid(recons, k, padding=2, pad_value=0.5).numpy(), make_grid(labels, k, padding=2, pad_value=0.5).numpy()


def generate_batch_compare_grid(batch_dict, s_mix_inbetween, label_mix_inbetween, recon_images, pred_labels, nclasses=3):
    """reference :36-63: rows = from / its reconstruction / between / synthesised / difference / reconstruction of to / to, for the image
    and for the labels."""
    image, between = batch_dict["image"].detach().cpu().float(), batch_dict["slice_between"].detach().cpu().float()
    n = between.size(0)

    def rows(c, mix, recon, scale):
        a, b = image[:, c, None].split(image.size(0) // 2, dim=0)
        ra, rb = recon.detach().cpu().float().split(recon.size(0) // 2, dim=0)
        ref, mix = between[:, c, None], mix.detach().cpu().float()
        return make_grid(torch.cat([a, ra, ref, mix, ref - mix, rb, b], dim=0) / scale, n, padding=2, pad_value=0.5).numpy()

    return rows(0, s_mix_inbetween, recon_images, 1.0), rows(1, label_mix_inbetween, pred_labels, float(nclasses))


class MultiChannelBaseTrainer(AEBaseTrainer):

    def _init_mask_loss(self, n_classes):
        self.nclasses = int(n_classes)
        self.mask_loss = DiceLoss(n_classes)

    # ---- the pieces of a step ------------------------------------------------------------------------------------------------------
    def _single_process(self):
        if self.dp is not None and self.dp.active:
            raise NotImplementedError("%s is single-process (data parallel is not built for the multi-channel trainers)" % type(self).__name__)

    def _head_losses(self, x, out, want_argmax):
        """(loss_ae, 0.1 * Dice, probs NHWC, argmax int32 or None) of one decoded sub-batch against its two-channel target."""
        loss_ae = self.get_loss(x[:, 0:1], out["image"], is_test=False)["loss_ae"]
        dice, probs, amax = self.mask_loss.from_logits(out["logits"], x[:, 1], want_argmax=want_argmax)
        return loss_ae, LABEL_WEIGHT * dice, probs, amax

    _training_after_step = False      # the host-side mode train() leaves the model in (what _step_core sets last)

    def _before_step(self):
        """Host-side work of train() that must not happen inside a captured step (device scalars the step reads)."""

    def train(self, batch_item, keep_predictions=True, eval_mode=False):
        """Thin wrapper: moves the batch, sets the mode, counts the step, then replays the captured step (``enable_step_graph``;
        ``AEBaseTrainer._graph_ok`` decides) or runs ``_step_core`` eagerly and keeps the predictions.  Only the two image tensors go to
        the step: both trainers mix at 0.5, so a batch's ``alpha_from`` / ``alpha_to`` would only be copied into the graph's inputs."""
        self._single_process()
        dev_batch = {k: self._to_device(batch_item[k]) for k in ("image", "slice_between")}
        if batch_item.get("_persistent"):
            dev_batch["_persistent"] = True          # LabelledTripletAugmenter(reuse_output=True): the buffer IS the graph's static input
        self._set_mode(not eval_mode)
        self._iters += 1
        self._note_batch(batch_item, "train")
        self._before_step()
        if self._graph_ok(keep_predictions, eval_mode):
            self._train_graphed(dev_batch)
            self._set_mode(self._training_after_step)      # a replay runs no Python: leave the mode the eager step leaves
            return
        r = self._step_core(dev_batch, eval_mode, want_argmax=keep_predictions)
        if keep_predictions:
            self._keep_step(r)

    def _keep(self, lat, mix, out_image, amax):
        s = mix["slice_inbetween_mix"].detach().cpu()
        self.train_predictions = {"z_mix": lat["z_mix"].detach().cpu(), "pred_alphas": torch.tensor([0.5]), "slice_inbetween_mix": s,
                                  "label_inbetween_mix": mix["label_inbetween_mix"].detach().cpu(), "slice_inbetween_05": s,
                                  "reconstruction": out_image.detach().cpu(), "pred_labels": amax.unsqueeze(1).long().cpu()}

    def _step_core(self, batch, eval_mode, want_argmax=False):
        """The plain step on device-resident inputs, written to be captured: no host read of a device value, every loss through ``_log``.
        ``between`` is encoded in EVAL mode behind the train-mode encoder pass; under capture the engine recomputes the eval-mode
        BatchNorm scale / shift in a launch of the step instead of taking them from its host cache."""
        x, between = batch["image"], batch["slice_between"]
        self.model.prepare_weights()
        z = self.model.encode(x)
        out = self.model.decode_logits(z)
        loss_ae, loss_labels, _, amax = self._head_losses(x, out, want_argmax)
        lat = self.get_latent_loss(reference=between, alpha_from=0.5, alpha_to=0.5, z=z.detach(), no_grad=True)      # leaves eval mode
        self._backward_and_step(loss_ae + loss_labels, eval_mode)
        self._log("loss_ae", loss_ae)
        self._log("loss_label", loss_labels)
        self._log("loss_latent_1", lat["loss_latent"])
        # reference :112-113: the logged mix is decoded with is_test=True AFTER the optimizer step -- new parameters, running statistics, no
        # BatchNorm update -- and nothing switches the model back: it is in eval mode when train() returns
        self._set_mode(False)
        return {"z": z, "lat": lat, "out": out, "amax": amax}

    def _keep_step(self, r):
        mix = self._get_mixup_image(z=r["z"].detach(), alpha_from=0.5, alpha_to=0.5, is_test=True)
        self._keep(r["lat"], mix, r["out"]["image"], r["amax"])

    # ---- eval wrappers -------------------------------------------------------------------------------------------------------------
    def decode(self, z, eval=True, clear_cache=False, chunk_size=16, **kwargs):
        """{'image', 'soft_probs', 'pred_labels' int64 [N, 1, H, W]} (reference :209-251)."""
        model = self._use_sr_model(kwargs.get("use_sr_model", False))
        z = self._to_device(z)
        model.train(not eval)
        if not eval:
            out = model.decode(z)
            out["pred_labels"] = out["soft_probs"].detach().argmax(dim=1, keepdim=True)
            return out
        per = model.max_elems_per_image("decode", tuple(z.shape[1:]))
        n_max = max(1, (1 << 28) // int(per))
        parts = [model.decode_labels(z[i:i + n_max]) for i in range(0, z.shape[0], n_max)]
        return parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}

    def predict(self, x, eval=True, chunk_size=16, clear_cache=False, **kwargs):
        z = self.encode(x, eval=eval, chunk_size=chunk_size, clear_cache=clear_cache, **kwargs)
        return self.decode(z, eval=eval, clear_cache=clear_cache, chunk_size=chunk_size, **kwargs)

    def _get_mixup_image(self, **kwargs):
        is_test = kwargs.get("is_test", False)
        z_mix = self._get_mixup_latent(**kwargs)
        r = self.decode(z_mix, eval=is_test)
        return {"z_mix": z_mix, "slice_inbetween_mix": r["image"], "soft_prob_mix": r["soft_probs"], "label_inbetween_mix": r["pred_labels"]}

    # ---- validation (reference :126-191) ---------------------------------------------------------------------------------------------
    def _validate_chunks(self, validation_batch, chunk_size=8):
        """Encode / decode the validation batch ``chunk_size`` images at a time (eval mode: same values as one pass) and log the mean of
        the chunks' reconstruction losses, as the reference does for batches of more than 16."""
        image = self._to_device(validation_batch["image"])
        chunks = list(torch.split(image, chunk_size, dim=0))
        zs, outs, l_ae, l_dist = [], [], 0.0, 0.0
        for xc in chunks:
            z = self.encode(xc, eval=True)
            o = self.decode(z, eval=True)
            ld = self.get_loss(xc[:, 0:1], o["image"], is_test=True, store_loss=False)
            l_ae, l_dist = l_ae + ld["loss_ae"], l_dist + ld["loss_ae_dist"]
            zs.append(z)
            outs.append(o)
        self._log("loss_ae", l_ae / len(chunks), True)
        self._log("loss_ae_dist", l_dist / len(chunks), True)
        res = {k: torch.cat([o[k] for o in outs], dim=0) for k in outs[0]}
        res["z"] = torch.cat(zs, dim=0)
        return res

    def validate(self, validation_batch, image_dict=None, frame_id=0, generate_images=True):
        self._single_process()
        self.model.eval()
        self._note_batch(validation_batch, "test")
        image = self._to_device(validation_batch["image"])
        if image.shape[0] > 16:
            r = self._validate_chunks(validation_batch, chunk_size=16)
            z = r["z"]
        else:
            z = self.encode(image, eval=True)
            r = self.decode(z, eval=True)
        loss = self.get_loss(image[:, 0:1], r["image"], is_test=True)["loss_ae"]
        with torch.no_grad():
            loss_labels = self.mask_loss(r["soft_probs"], image[:, 1])          # reference :139: not weighted here
        lat = self.get_latent_loss(reference=self._to_device(validation_batch["slice_between"]), z=z, alpha_from=0.5, alpha_to=0.5, no_grad=True)
        self.test_predictions = {"z": z.detach().cpu(), "img_recons": r["image"].detach().cpu(), "z_device": z.device,
                                 "pred_labels": r["pred_labels"].detach().cpu()}
        grid = label_grid = None
        if generate_images:
            grid, label_grid = generate_recon_grid(validation_batch["image"][:, 0:1], validation_batch["image"][:, 1:2],
                                                   self.test_predictions["img_recons"], self.test_predictions["pred_labels"])
        self._log("loss_ae", loss, True)
        self._log("loss_label", loss_labels, True)
        self._log("loss_latent_1", lat["loss_latent"], True)
        self.save_best_val_model()
        result = {"img_grid_recons": grid, "loss_ae": self.losses_test["loss_ae"][-1], "pred_label_grid": label_grid}
        if image_dict is not None:
            result.update(self._generate_val_volumes(image_dict, frame_id=frame_id))
        from ..base_trainer import _check_watchdogs
        _check_watchdogs(self, "validate")      # behind the whole-volume previews too: nothing of this call is handed out unchecked
        return result

    def _generate_val_volumes(self, image_dict, frame_id):
        """Whole-volume validation previews with label scores.  ``image_dict[p_id]``: {'image' [t,z,y,x] in [0,1], 'labels' [t,z,y,x] class
        ids, 'patient_id', 'spacing' (z,y,x)} (``data_device.load_labelled_image_dict``).  Per patient, frame ``frame_id`` (clipped to the
        last frame) of the image and of its label map is padded / centre-cropped to ``eval_patch_size`` (default ``width``) with one
        geometry (label padding 0 = background), every 2nd slice kept and the held-out slices AND label maps synthesised at alpha 0.5
        (``evaluate.common.create_super_volume(labels=)``); the synthesised label volume is scored on the device against the full label
        volume beside the nearest-slice baseline (``evaluate.seg_metrics.score_label_supervolume``).  Returns {'synthesized_vols',
        'synthesized_label_vols': {p_id: comparison grid (labels / nclasses)}, 'alphas', 'label_scores': {p_id: {'model', 'nearest'}}};
        the volumes behind the grids stay in ``self.val_volume_predictions[p_id]`` ('image', 'labels': the cropped frame; 'upsampled_image',
        'upsampled_labels': the super-volume).  The scores are not losses: they never enter ``losses_test``."""
        from ...evaluate.common import create_super_volume
        from ...evaluate.evaluate_image import create_compare_image
        from ...evaluate.find_best_model import adjust_and_center_crop
        from ...evaluate.seg_metrics import score_label_supervolume
        eval_patch_size = self.args.get("eval_patch_size", self.args["width"])
        vols, label_vols, alphas, scores, kept = {}, {}, {}, {}, {}
        for p_id, data in image_dict.items():
            if tuple(data["labels"].shape) != tuple(data["image"].shape):
                raise ValueError("patient %s: the labels %s do not match the image %s" % (p_id, tuple(data["labels"].shape), tuple(data["image"].shape)))
            f_id = min(int(frame_id), int(data["image"].shape[0]) - 1)
            vol = torch.from_numpy(np.ascontiguousarray(adjust_and_center_crop(data["image"][f_id], eval_patch_size)))
            lab = torch.from_numpy(np.ascontiguousarray(adjust_and_center_crop(data["labels"][f_id], eval_patch_size)))      # float32: small integers, exact
            out = create_super_volume(self, vol, alpha_range=[0.5], downsample_steps=2, generate_inbetween_slices=True, labels=lab)
            up_img, up_lab = out["upsampled_image"].detach().cpu(), out["upsampled_labels"].detach().cpu()
            vols[p_id] = create_compare_image(vol.numpy(), up_img.numpy())
            label_vols[p_id] = create_compare_image(lab.numpy() / self.nclasses, up_lab.float().numpy() / self.nclasses)
            alphas[p_id] = out["pred_alphas"].squeeze()
            scores[p_id] = score_label_supervolume(self, vol, lab, 2, data["spacing"])
            kept[p_id] = {"image": vol, "labels": lab, "upsampled_image": up_img, "upsampled_labels": up_lab}
        self.val_volume_predictions = kept
        return {"synthesized_vols": vols, "synthesized_label_vols": label_vols, "alphas": alphas, "label_scores": scores}

    # ---- epoch hooks (reference :253-276) --------------------------------------------------------------------------------------------
    def generate_train_images(self, **kwargs):
        if not self._is_writer() or self.train_predictions is None:
            return
        p = self.train_predictions
        grid, label_grid = generate_batch_compare_grid(kwargs.get("batch_item"), p["slice_inbetween_mix"], p["label_inbetween_mix"],
                                                       p["reconstruction"], p["pred_labels"])
        fname = os.path.join(self.args["dir_images"], "train_image_e{:03d}_{}.png".format(kwargs.get("epoch"), self.iters))
        save_image_grid(grid, fname)
        save_image_grid(label_grid, fname.replace("_image_", "_pred_labels_"))

    def end_epoch_processing(self, **kwargs):
        val = kwargs.get("val_result_dict") or {}
        super().end_epoch_processing(**kwargs)          # advances self.epoch (the reference adds a second increment here: a slip, not kept)
        if not self._is_writer():
            return
        epoch, images = kwargs.get("epoch"), self.args["dir_images"]
        if val.get("pred_label_grid") is not None:
            save_image_grid(val["pred_label_grid"], os.path.join(images, "val_pred_labels_e{:03d}.png".format(epoch)))
        # whole-volume previews: val_image_e###_p###.png is the base class's; the label grid beside it, and every score table of every patient in
        # one file per epoch, keys "p###/model/dice", "p###/nearest/hd95", ... ([N][C] as evaluate.seg_metrics returns them)
        for p_id, grid in (val.get("synthesized_label_vols") or {}).items():
            save_image_grid(grid, os.path.join(images, "val_labels_e{:03d}_p{:03d}.png".format(epoch, int(p_id))))
        if val.get("label_scores"):
            np.savez(os.path.join(images, "val_label_scores_e{:03d}.npz".format(epoch)),
                     **{"p{:03d}/{}/{}".format(int(p_id), who, k): np.asarray(v) for p_id, both in val["label_scores"].items()
                        for who, table in both.items() for k, v in table.items()})


def mean_label_dice(label_scores):
    """(model, nearest): the mean Dice over classes and patients of ``validate(image_dict=...)['label_scores']``."""
    return tuple(float(np.mean([np.mean(both[who]["dice"]) for both in label_scores.values()])) for who in ("model", "nearest"))


class MultiChannelTrainer(MultiChannelBaseTrainer):

    def __init__(self, args, ae, max_grad_norm=0, model_file=None, eval_mode=False, **kwargs):
        super(MultiChannelTrainer, self).__init__(args, ae, max_grad_norm, model_file, eval_mode, **kwargs)
        self._init_mask_loss(args["nclasses"])


class MultiChannelCAISRTrainer(CombinedStepMixin, MultiChannelBaseTrainer):

    def __init__(self, args, ae, max_grad_norm=0, model_file=None, eval_mode=False, **kwargs):
        super(MultiChannelCAISRTrainer, self).__init__(args, ae, max_grad_norm, model_file, eval_mode, **kwargs)
        self._init_mask_loss(args["nclasses"])

    _training_after_step = True
    train = MultiChannelBaseTrainer.train          # not CombinedStepMixin's, which comes first in the MRO: two-channel batches, labels kept

    def _before_step(self):
        self._lambda_tensor()          # the synthesis weight reaches its device scalar here: _weigh_and_log then launches nothing for it

    def _step_core(self, batch, eval_mode, want_argmax=False):
        """The combined step on device-resident inputs, written to be captured (see ``MultiChannelBaseTrainer._step_core``)."""
        x, between = batch["image"], batch["slice_between"]
        self.model.prepare_weights()
        z = self.model.encode(x)
        lat = self.get_latent_loss(reference=between, alpha_from=0.5, alpha_to=0.5, z=z.detach(), no_grad=True)      # leaves eval mode
        self._set_mode(not eval_mode)
        z_mix = ops.lerp_mix(z, 0.5, 0.5)
        out, mix = self.model.decode_multi([z, z_mix])          # dec(z) then dec(z_mix): two BatchNorm statistic groups, in that order
        loss_ae, loss_labels, _, amax = self._head_losses(x, out, want_argmax)
        loss_extra, amax_mix = self._extra_from_logits(between, mix, want_argmax, is_test=False)
        self._backward_and_step(loss_ae + loss_extra + loss_labels, eval_mode)
        self._log("loss_ae", loss_ae)
        self._log("loss_label", loss_labels)
        self._log("loss_latent_1", lat["loss_latent"])
        return {"lat": lat, "mix": mix, "out": out, "amax": amax, "amax_mix": amax_mix}

    def _keep_step(self, r):
        self._keep(r["lat"], {"slice_inbetween_mix": r["mix"]["image"], "label_inbetween_mix": r["amax_mix"].unsqueeze(1).long()},
                   r["out"]["image"], r["amax"])

    def _weigh_and_log(self, loss_image, loss_labels, is_test):
        w = self._lambda_tensor()
        loss_image, loss_labels = w * loss_image, w * loss_labels
        total = loss_image + loss_labels
        self._log("loss_ae_extra", total, is_test)
        self._log("loss_ae_dist_extra", loss_image, is_test)
        self._log("loss_ae_dist_labels", loss_labels, is_test)
        return total

    def _extra_from_logits(self, slice_between, mix, want_argmax, is_test):
        """The synthesis terms of the training step (reference :364-414) with the Dice term taken from the logits."""
        loss_image = CombinedStepMixin.get_extra_image_loss(self, slice_between[:, 0:1], mix["image"], is_test=is_test)
        dice, _, amax = self.mask_loss.from_logits(mix["logits"], slice_between[:, 1], want_argmax=want_argmax)
        return self._weigh_and_log(loss_image, dice, is_test), amax

    def get_extra_image_loss(self, reference, synthesized, soft_probs_synthesized):
        """reference :388-414: (image loss on channel 0 -- LPIPS or MSE (+ LapLoss) --, Dice of the soft probabilities against channel 1)."""
        loss_image = CombinedStepMixin.get_extra_image_loss(self, reference[:, 0:1], synthesized, is_test=not torch.is_grad_enabled())
        return loss_image, self.mask_loss(soft_probs_synthesized, reference[:, 1])

    def get_extra_loss(self, slice_between, s_between_mix, soft_probs_between_mix, is_test=False):
        """reference :364-386 on soft probabilities (validation; the training step uses ``_extra_from_logits``)."""
        ctxm = torch.no_grad() if is_test else torch.enable_grad()
        with ctxm:
            loss_image, loss_labels = self.get_extra_image_loss(slice_between, s_between_mix, soft_probs_between_mix)
        return self._weigh_and_log(loss_image, loss_labels, is_test)

    def validate(self, validation_batch, image_dict=None, frame_id=0, generate_images=True):
        res = super().validate(validation_batch, image_dict=image_dict, frame_id=frame_id, generate_images=generate_images)
        z = self.test_predictions["z"].to(self.test_predictions["z_device"])
        r = self._get_mixup_image(z=z, alpha_from=0.5, alpha_to=0.5, is_test=True)
        self.get_extra_loss(self._to_device(validation_batch["slice_between"]), r["slice_inbetween_mix"], r["soft_prob_mix"], is_test=True)
        self.save_best_val_model()
        return res

    def save_best_val_model(self, **kwargs):
        MultiChannelBaseTrainer.save_best_val_model(self)
        if self._best_now("loss_ae_extra"):
            self.save_models(os.path.join(self.args["dir_models"], "caisr.models"), self.epoch + 1)
