"""-m gpu: whole-volume validation of the multi-channel trainers -- ``validate(image_dict=...)`` previews held-out slices AND label maps of
in-memory patients and scores the synthesised label maps on the device (``MultiChannelBaseTrainer._generate_val_volumes``), and the command
line that feeds it (``--val_volumes_dir`` with ``--val_labels_dir``).  Every comparison is between two runs of the same arithmetic: exact,
no pixel excluded."""
import os

import numpy as np
import pytest
import torch

import test_multichannel_golden as tm
from test_gpu_multichannel import make_trainer

pytestmark = pytest.mark.gpu
BASE_KEYS = ["img_grid_recons", "loss_ae", "pred_label_grid"]
NEW_KEYS = ["alphas", "label_scores", "synthesized_label_vols", "synthesized_vols"]
TEST_KEYS = ["loss_ae", "loss_ae_dist", "loss_ae_dist_extra", "loss_ae_dist_labels", "loss_ae_extra", "loss_label", "loss_latent_1"]


def patient(T, Z, H, W, seed):
    """image [T, Z, H, W] in [0, 1] and a label map of nested blobs (classes 0 ... 3) that drift and shrink from slice to slice"""
    g = np.random.RandomState(seed)
    zz, yy, xx = np.meshgrid(np.arange(float(Z)), np.arange(float(H)), np.arange(float(W)), indexing="ij")
    frames, labels = [], []
    for t in range(T):
        field = np.exp(-((yy - H / 2 - 0.6 * zz + t) ** 2 + (xx - W / 2 + 0.5 * zz) ** 2) / (2 * (6.0 + 0.3 * zz) ** 2))
        labels.append(np.floor(4 * 0.999 * field).astype(np.uint8))
        frames.append(np.clip(field + 0.05 * g.rand(Z, H, W), 0, 1).astype(np.float32))
    return {"image": np.stack(frames), "labels": np.stack(labels), "spacing": np.array([5.0, 1.4, 1.4])}


def same_table(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f"), k


def test_validate_previews_and_scores_whole_labelled_volumes():
    from superresolution_aniso_mri_amd.evaluate import common as ec
    from superresolution_aniso_mri_amd.evaluate.evaluate_image import create_compare_image
    from superresolution_aniso_mri_amd.evaluate.find_best_model import adjust_and_center_crop
    from superresolution_aniso_mri_amd.evaluate.seg_metrics import score_label_supervolume
    rec = tm.load("step_k3_mc_caisr_mse.npz")
    tr = make_trainer("ae_combined", "mse", {k[3:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("p0/")})
    batch = {"image": torch.from_numpy(rec["image_0"]), "slice_between": torch.from_numpy(rec["between_0"])}
    tr.train(batch, keep_predictions=False)
    d = {7: dict(patient(2, 7, 36, 30, 1), patient_id="patient007"), 12: dict(patient(1, 8, 30, 36, 2), patient_id="patient012")}
    res = tr.validate(batch, image_dict=d, frame_id=1)
    assert sorted(res) == sorted(BASE_KEYS + NEW_KEYS)
    assert sorted(tr.losses_test.keys()) == TEST_KEYS and all(len(v) == 1 for v in tr.losses_test.values())          # the scores are no losses
    for k in NEW_KEYS:
        assert sorted(res[k]) == [7, 12], k
    for p_id, data in d.items():
        f = 1 if p_id == 7 else 0          # frame_id beyond the last frame means the last frame
        vol = torch.from_numpy(np.ascontiguousarray(adjust_and_center_crop(data["image"][f], 32)))
        lab = torch.from_numpy(np.ascontiguousarray(adjust_and_center_crop(data["labels"][f], 32)))
        Z = vol.shape[0]
        assert tuple(vol.shape) == tuple(lab.shape) == (Z, 32, 32) and set(np.unique(lab.numpy())) == {0.0, 1.0, 2.0, 3.0}
        # one geometry for both: the label map still lies on its image (the image is the field the labels were cut from, plus 5 % noise)
        assert bool(((vol >= 0.5) == (lab >= 2))[(vol - 0.5).abs() > 0.06].all())
        kept = tr.val_volume_predictions[p_id]
        assert torch.equal(kept["image"], vol) and torch.equal(kept["labels"], lab)
        direct = ec.create_super_volume(tr, vol, alpha_range=[0.5], downsample_steps=2, generate_inbetween_slices=True, labels=lab)
        up = kept["upsampled_labels"]
        assert up.dtype == direct["upsampled_labels"].dtype and torch.equal(up, direct["upsampled_labels"]) and tuple(up.shape) == (Z, 32, 32)
        assert torch.equal(kept["upsampled_image"], direct["upsampled_image"])
        assert np.array_equal(res["synthesized_label_vols"][p_id], create_compare_image(lab.numpy() / 4, up.float().numpy() / 4))
        assert np.array_equal(res["synthesized_vols"][p_id], create_compare_image(vol.numpy(), direct["upsampled_image"].numpy()))
        assert res["synthesized_label_vols"][p_id].shape == res["synthesized_vols"][p_id].shape
        # class ids 0 ... 3 over nclasses = 4; the difference row of the grid may reach -0.75
        assert -0.75 <= res["synthesized_label_vols"][p_id].min() and res["synthesized_label_vols"][p_id].max() <= 0.75
        assert torch.equal(res["alphas"][p_id], direct["pred_alphas"].squeeze())
        # slot order: kept slices hold the RECONSTRUCTED label maps, a remainder slice the original one
        remain = (Z - 1) % 2
        assert remain == (1 if p_id == 12 else 0)
        body = Z - remain
        recon = tr.predict(torch.stack([vol[:body:2], lab[:body:2]], dim=1))["pred_labels"][:, 0].cpu()
        assert torch.equal(up[:body:2].long(), recon)
        if remain:
            assert torch.equal(up[-1].float(), lab[-1])
        # the scores: the model beside the nearest-slice baseline, the [N][C] tables as the scoring function returns them
        want = score_label_supervolume(tr, vol, lab, 2, data["spacing"])
        got = res["label_scores"][p_id]
        assert sorted(got) == ["model", "nearest"]
        for who in got:
            same_table(got[who], want[who])
            assert got[who]["dice"].shape == (1, 3) and bool(np.isfinite(got[who]["dice"]).all())
        assert float(got["nearest"]["dice"].min()) > 0.3          # neighbouring slices of drifting blobs overlap: the baseline is no zero
    # without image_dict: exactly today's result and today's logged keys
    tr.reset_losses()
    res = tr.validate(batch)
    assert sorted(res) == BASE_KEYS
    assert sorted(k for k, v in tr.losses_test.items() if len(v)) == TEST_KEYS


def test_val_labels_dir_on_the_command_line(tmp_path, capsys):
    from superresolution_aniso_mri_amd import train_aesr
    data, labs = tmp_path / "vols", tmp_path / "labels"
    data.mkdir()
    labs.mkdir()
    for n, seed in ((3, 5), (4, 6)):
        p = patient(1, 8 - (n % 2), 40, 36, seed)
        np.save(str(data / ("vol%d.npy" % n)), p["image"][0])
        np.save(str(labs / ("vol%d.npy" % n)), p["labels"][0])
    out = str(tmp_path / "expers")
    tr = train_aesr.main(["--dataset=ACDCLBL", "--model=ae_combined", "--batch_size=4", "--test_batch_size=4", "--latent=16", "--latent_width=8",
                          "--width=32", "--depth=8", "--downsample_steps=2", "--epochs=1", "--lr=0.001", "--ex_loss_weight1=0.05", "--exper_id=v",
                          "--output_dir=" + out, "--volumes_dir=" + str(data), "--labels_dir=" + str(labs), "--aug_patch_size=36",
                          "--val_volumes_dir=" + str(data), "--val_labels_dir=" + str(labs), "--iters_per_epoch=4",
                          "--image_mix_loss_func=mse", "--epoch_threshold=0"])
    images = os.path.join(out, "v", "log_images")
    for p_id in (3, 4):
        for kind in ("image", "labels"):
            assert os.path.isfile(os.path.join(images, "val_%s_e001_p%03d.png" % (kind, p_id))), (kind, p_id)
    scores = np.load(os.path.join(images, "val_label_scores_e001.npz"))
    for p_id in (3, 4):
        for who in ("model", "nearest"):
            dice = scores["p%03d/%s/dice" % (p_id, who)]
            assert dice.shape == (1, 3) and bool(np.isfinite(dice).all()) and dice.min() >= 0 and dice.max() <= 1
            assert scores["p%03d/%s/hd95" % (p_id, who)].shape == (1, 3)
    assert sorted(tr.mean_losses_test.keys()) == sorted(TEST_KEYS)          # no score among the losses
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("epoch")]
    assert len(line) == 1 and "label dice" in line[0] and "nearest slice" in line[0]
