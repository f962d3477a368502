"""-m gpu: the captured training step of ``MultiChannelTrainer`` / ``MultiChannelCAISRTrainer`` (``enable_step_graph``).

A replayed step is the eager step launch for launch, so every comparison here is between two runs of the same arithmetic and is exact:
losses equal as floats, every ``state_dict`` entry (BatchNorm running statistics and ``num_batches_tracked`` included) and the optimizer's
step count bit for bit, the host-side train / eval flag after every step.  The fixtures ``step_k3_mc_*.npz`` are pinned to the reference's
own ``train()`` by tests/test_gpu_multichannel.py, so "equal to eager" is "equal to the reference" within that file's bounds.

Both trainers encode ``slice_between`` in EVAL mode inside the step, behind a train-mode encoder pass that has just moved the running
statistics: a replay that took the eval-mode BatchNorm scale / shift from the host cache (or baked the capture step's into the graph) would
log another ``loss_latent_1`` from the second replay on -- the loss lists below would differ."""
import os

import numpy as np
import pytest
import torch

import memguard as mg
import test_multichannel_golden as tm
from test_gpu_multichannel import make_trainer

pytestmark = pytest.mark.gpu
TAGS = ["plain", "caisr_mse", "caisr_lpips"]
PLAIN_KEYS = ["loss_ae", "loss_ae_dist", "loss_label", "loss_latent_1"]
CAISR_KEYS = PLAIN_KEYS + ["loss_ae_extra", "loss_ae_dist_extra", "loss_ae_dist_labels"]
KEPT_KEYS = ["label_inbetween_mix", "pred_alphas", "pred_labels", "reconstruction", "slice_inbetween_05", "slice_inbetween_mix", "z_mix"]


def load(tag):
    return tm.load("step_k3_mc_%s.npz" % tag)


def trainer_of(tag, rec, **over):
    return make_trainer("ae" if tag == "plain" else "ae_combined", "perceptual" if tag.endswith("lpips") else "mse",
                        {k[3:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("p0/")}, **over)


def batch_of(rec, k):
    return {"image": torch.from_numpy(rec["image_%d" % k]), "slice_between": torch.from_numpy(rec["between_%d" % k])}


def assert_same_state(eager, graphed, steps):
    a, b = eager.model.state_dict(), graphed.model.state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(mg.bits(a[k]), mg.bits(b[k])), k
    assert any("num_batches_tracked" in k for k in a)
    for tr in (eager, graphed):
        assert float(tr.opt_ae.dev_state[0]) == steps
    assert torch.equal(mg.bits(eager.opt_ae.flat_m), mg.bits(graphed.opt_ae.flat_m))
    assert torch.equal(mg.bits(eager.opt_ae.flat_v), mg.bits(graphed.opt_ae.flat_v))


def assert_same_losses(eager, graphed, keys, n):
    assert list(eager.losses.keys()) == list(graphed.losses.keys()) and sorted(eager.losses.keys()) == sorted(keys)
    for k in keys:
        a, b = eager.losses[k].floats(), graphed.losses[k].floats()
        assert len(a) == len(b) == n and all(np.isfinite(a)), k
        assert a == b, (k, a, b)


@pytest.mark.parametrize("tag", TAGS)
def test_replayed_steps_are_the_eager_steps_bit_for_bit(tag):
    rec = load(tag)
    eager, graphed = trainer_of(tag, rec), trainer_of(tag, rec)
    graphed.enable_step_graph(eager_steps=1)
    for step in range(6):          # graphed: one eager step, the capture step, four replays
        for tr in (eager, graphed):
            tr.train(batch_of(rec, step % 3), keep_predictions=False)
        assert eager.model.training == graphed.model.training == (tag != "plain"), step
        assert all(m.training == graphed.model.training for m in graphed.model.modules()), step
    assert len(graphed._graphs) == 1 and not getattr(eager, "_graph_enabled", False)
    assert_same_losses(eager, graphed, PLAIN_KEYS if tag == "plain" else CAISR_KEYS, 6)
    assert_same_state(eager, graphed, 6)
    assert eager.iters == graphed.iters == 7 and graphed.train_predictions is None
    # the replays really trained: the logged latent loss of the eval-mode pass moves from step to step
    assert len(set(graphed.losses["loss_latent_1"].floats())) == 6


@pytest.mark.parametrize("tag", ["plain", "caisr_mse"])
def test_eval_after_replayed_steps_sees_the_replayed_state(tag):
    """validate() / predict() behind an eager step (fills the host caches), right behind the capture step and behind replays only: each
    equals the same call on an all-eager trainer, bit for bit."""
    rec = load(tag)
    eager, graphed = trainer_of(tag, rec), trainer_of(tag, rec)
    graphed.enable_step_graph(eager_steps=1)
    eager.WATCHDOG_EVERY = graphed.WATCHDOG_EVERY = 2          # the periodic watchdog poll (a device sync) on every other step
    val = batch_of(rec, 2)
    got = {"eager": [], "graphed": []}

    def look(tr):
        loss = tr.validate(val, generate_images=False)["loss_ae"]
        logged = {k: v[-1] for k, v in tr.losses_test.items()}
        return loss, logged, {k: v.clone() for k, v in tr.predict(val["image"]).items()}

    for name, tr in (("eager", eager), ("graphed", graphed)):
        for step in range(6):
            if step in (1, 2):
                got[name].append(look(tr))
            tr.train(batch_of(rec, step % 3), keep_predictions=False)
        got[name].append(look(tr))
    assert len(graphed._graphs) == 1
    for (la, ta, pa), (lb, tb, pb) in zip(got["eager"], got["graphed"]):
        assert float(la) == float(lb) and ta == tb
        assert sorted(pa) == sorted(pb) == ["image", "pred_labels", "soft_probs"]
        for k in pa:
            assert torch.equal(mg.bits(pa[k]), mg.bits(pb[k])), k
    assert not torch.equal(got["graphed"][1][2]["image"], got["graphed"][2][2]["image"])          # the state moved between the looks
    assert not torch.equal(got["graphed"][0][2]["image"], got["graphed"][1][2]["image"])
    assert_same_state(eager, graphed, 6)


@pytest.mark.parametrize("tag", ["plain", "caisr_mse"])
def test_a_step_that_keeps_its_predictions_runs_eagerly_between_replays(tag):
    rec = load(tag)
    eager, graphed = trainer_of(tag, rec), trainer_of(tag, rec)
    graphed.enable_step_graph(eager_steps=1)
    for step in range(7):
        keep = step == 4          # behind two replays, two more follow
        for tr in (eager, graphed):
            tr.train_predictions = None
            tr.train(batch_of(rec, step % 3), keep_predictions=keep)
        assert eager.model.training == graphed.model.training == (tag != "plain")
        if keep:
            a, b = eager.train_predictions, graphed.train_predictions
            assert sorted(a) == sorted(b) == KEPT_KEYS
            for k in KEPT_KEYS:
                assert torch.equal(mg.bits(a[k]), mg.bits(b[k])), k
            assert b["pred_labels"].dtype == torch.int64 and b["label_inbetween_mix"].dtype == torch.int64
        else:
            assert graphed.train_predictions is None
    assert len(graphed._graphs) == 1
    assert_same_losses(eager, graphed, PLAIN_KEYS if tag == "plain" else CAISR_KEYS, 7)
    assert_same_state(eager, graphed, 7)


def labelled_volumes(n=2, Z=6):
    zz, yy, xx = np.meshgrid(np.arange(float(Z)), np.arange(40.0), np.arange(36.0), indexing="ij")
    out = []
    for cy, cx in ((19.0, 17.0), (21.0, 18.5), (18.0, 19.0))[:n]:
        field = np.exp(-((yy - cy - 0.5 * zz) ** 2 + (xx - cx + 0.4 * zz) ** 2) / (2 * 8.0 ** 2))
        out.append((field.astype(np.float32), np.floor(4 * 0.999 * field).astype(np.uint8)))
    return out


def test_persistent_augmenter_batches_are_the_static_input():
    """``LabelledTripletAugmenter(reuse_output=True)`` writes every batch into one buffer: the graph adopts it (no copy node, no clone) and
    each replay reads the batch that was assembled last -- never an earlier one."""
    from superresolution_aniso_mri_amd.data_device import LabelledTripletAugmenter
    rec = load("caisr_mse")
    vols = labelled_volumes()
    aug = LabelledTripletAugmenter([v for v, _ in vols], [l for _, l in vols], 32, 36, rs=np.random.RandomState(11), device="cuda")
    eager, graphed = trainer_of("caisr_mse", rec), trainer_of("caisr_mse", rec)
    graphed.enable_step_graph(eager_steps=1)
    seen = []
    for step in range(6):          # graphed: one eager step, the capture step, four replays
        batch = aug.next_batch(4, reuse_output=True)
        assert batch["_persistent"] and tuple(batch["image"].shape) == (8, 2, 32, 32) and tuple(batch["slice_between"].shape) == (4, 2, 32, 32)
        copy = {k: batch[k].clone() for k in ("image", "slice_between")}
        seen.append(mg.bits(copy["image"]))
        graphed.train(batch, keep_predictions=False)
        eager.train(copy, keep_predictions=False)
    assert len(graphed._graphs) == 1
    (_, static, _), = graphed._graphs.values()
    both = aug._out[(4, 32)][0]
    assert static["image"].data_ptr() == both.data_ptr() == batch["image"].data_ptr()
    assert static["slice_between"].data_ptr() == both[8:].data_ptr() == batch["slice_between"].data_ptr()
    assert sorted(static) == ["image", "slice_between"]
    assert all(not torch.equal(seen[i], seen[i + 1]) for i in range(5))          # six different batches went through one address
    assert_same_losses(eager, graphed, CAISR_KEYS, 6)
    assert_same_state(eager, graphed, 6)


COMMON = ["--dataset=ACDCLBL", "--model=ae_combined", "--batch_size=4", "--test_batch_size=4", "--latent=16", "--latent_width=8", "--width=32",
          "--depth=8", "--downsample_steps=2", "--epochs=2", "--lr=0.001", "--ex_loss_weight1=0.05", "--iters_per_epoch=4",
          "--image_mix_loss_func=mse", "--epoch_threshold=0"]


def run_pair(tmp_path, extra):
    from superresolution_aniso_mri_amd import train_aesr
    out, sd, trainers = str(tmp_path / "expers"), {}, {}
    for name, flags in (("eager", []), ("graph", ["--use_step_graph"])):
        trainers[name] = train_aesr.main(COMMON + ["--exper_id=" + name, "--output_dir=" + out] + extra + flags)
        sd[name] = torch.load(os.path.join(out, name, "models", "2.models"), map_location="cpu")["model_dict_ae"]
    # eight steps: 1, 2 and 4 use up the eager warm-up, 3 and 7 keep their predictions for the epoch's images, 5 captures, 6 and 8 replay
    assert len(trainers["graph"]._graphs) == 1 and not getattr(trainers["eager"], "_graph_enabled", False)
    assert trainers["eager"].iters == trainers["graph"].iters == 9
    assert list(sd["eager"].keys()) == list(sd["graph"].keys())
    for k in sd["eager"]:
        assert torch.equal(mg.bits(sd["eager"][k]), mg.bits(sd["graph"][k])), k
    for k, v in trainers["eager"].mean_losses.items():
        assert v == trainers["graph"].mean_losses[k], k
    return trainers


def test_use_step_graph_on_the_command_line_trains_the_same_model(tmp_path):
    trainers = run_pair(tmp_path, ["--synthetic"])
    assert type(trainers["graph"]).__name__ == "MultiChannelCAISRTrainer"


def test_use_step_graph_with_labelled_volumes_reads_the_augmenters_buffer(tmp_path):
    """``--volumes_dir`` / ``--labels_dir`` with ``--use_step_graph``: training batches arrive in the augmenter's persistent buffer, which is
    the graph's static input; the validation batch keeps tensors of its own."""
    from superresolution_aniso_mri_amd.data_device import LabelledTripletAugmenter
    data, labs = tmp_path / "vols", tmp_path / "labels"
    data.mkdir()
    labs.mkdir()
    for n, (v, l) in enumerate(labelled_volumes(Z=8)):
        np.save(str(data / ("vol%d.npy" % n)), v)
        np.save(str(labs / ("vol%d.npy" % n)), l)
    seen, keep = [], LabelledTripletAugmenter.next_batch

    def spy(self, *a, **k):
        out = keep(self, *a, **k)
        seen.append((bool(k.get("raw", False)), bool(out.get("_persistent")), out["image"].data_ptr()))
        return out

    LabelledTripletAugmenter.next_batch = spy
    try:
        trainers = run_pair(tmp_path, ["--volumes_dir=" + str(data), "--labels_dir=" + str(labs), "--aug_patch_size=36"])
    finally:
        LabelledTripletAugmenter.next_batch = keep
    runs = [seen[:9], seen[9:]]
    assert [len(r) for r in runs] == [9, 9] and all(r[0][0] and not r[0][1] for r in runs)          # the validation batch: raw, its own tensors
    assert not any(p for _, p, _ in runs[0][1:]) and all(p for _, p, _ in runs[1][1:])
    assert len({ptr for _, _, ptr in runs[1][1:]}) == 1
    (_, static, _), = trainers["graph"]._graphs.values()
    assert static["image"].data_ptr() == runs[1][1][2]
