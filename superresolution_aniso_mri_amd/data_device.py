"""On-device batch assembly + augmentation for ae_combined training.

The reference feeds the step from a 2-worker numpy DataLoader: per sample a [3,H,W] triplet (from, to, between) is gathered
from a 4-D volume (datasets/ACDC/data4d_simple.py:191-240), padded / centre-cropped to ``aug_patch_size``, randomly cropped
to ``width``, passed through a random sigmoid intensity curve and rotated by a random multiple of 90 degrees
(train_cardiac_aesr.py:83-96; datasets/shared_transforms.py), then collated and re-laid out by ``prepare_batch_pairs``.
At several thousand slices per second that pipeline is the bottleneck.  Here the volumes live in HBM and ONE kernel launch
(``aesr_triplet_assemble``) produces the step's ``image`` [2B,1,W,W] / ``slice_between`` [B,1,W,W] tensors.  The random
numbers are drawn on the host from a numpy ``RandomState`` in the reference's order, so a single-worker reference loader with
the same state yields the same batch."""
import numpy as np
import torch

from . import _hip
from ._hip import check, lib, ptr, stream


def get_random_adjacent_slice(slice_id, num_slices, rs, step=1):
    """datasets/common.py:34-43"""
    last = num_slices - 1
    if slice_id + step > last:
        return slice_id - step
    if slice_id == 0:
        return step
    if slice_id - step < 0:
        return slice_id + step
    # rs.choice([a, b]) draws ONE rs.randint(0, 2) (numpy legacy RandomState.choice without p): the same stream position and result
    # at a third of the host time (8.6 -> 2.7 us per draw; the training loop makes ~10 draws per sample)
    return (slice_id - step, slice_id + step)[int(rs.randint(0, 2))]


def rescale_intensities(vol, percs=(1, 99)):
    """datasets/ACDC/data.py:151-160: percentile window -> [0, 1]."""
    lo, hi = np.percentile(vol, percs)
    lo = 0 if np.isnan(lo) else lo
    hi = 1 if np.isnan(hi) else hi
    return ((vol.astype(np.float32) - lo) / (hi - lo)).clip(0, 1)


NEW_SPACING = (1.4, 1.4)      # CardiacImage.new_spacing[1:] of the reference (datasets/cardiac_image.py:49): the in-plane training spacing


def _resample_to(arr, spacing_zyx, new_spacing, f):
    """``CardiacImage(resample=True)`` (datasets/cardiac_image.py:80-82, 102-104): in-plane resampling of a [Z,H,W] / [T,Z,H,W] array to
    ``new_spacing`` on the device (datasets/common.py; all slices in one launch), BEFORE the intensities are rescaled."""
    from .datasets.common import apply_2d_zoom_3d, apply_2d_zoom_4d
    if spacing_zyx is None:
        raise ValueError("%s: resample=True needs the volume's spacing, and a .npy file carries none (use .nii / .mha)" % f)
    fn = apply_2d_zoom_3d if arr.ndim == 3 else apply_2d_zoom_4d
    return fn(np.asarray(arr, dtype=np.float32), spacing_zyx, NEW_SPACING if new_spacing is None else new_spacing)


def _check_brain_options(thick_slices, downsample_steps, resample):
    if thick_slices is None and downsample_steps is None:
        return False
    if downsample_steps is None or int(downsample_steps) < 1:
        raise ValueError("thick_slices / downsample_steps: downsample_steps=%r must be a positive integer" % (downsample_steps,))
    if thick_slices is not None and not float(thick_slices) > 0:
        raise ValueError("thick_slices=%r must be a positive thickness (None for volumes that are blurred already)" % (thick_slices,))
    if resample:
        raise ValueError("resample (the cardiac in-plane step) and thick_slices / downsample_steps (the brain through-plane step) exclude each other")
    return True


def load_volume_dir(path, resample=False, new_spacing=None, thick_slices=None, downsample_steps=None, percs=(0, 100), device="cuda"):
    """All volumes of a directory (.npy, .nii, .nii.gz, .mha, .mhd; 3-D [Z,H,W] or 4-D [T,Z,H,W] -> one volume per frame),
    each rescaled to [0,1] by its 1st / 99th percentile when it is not already in that range.  ``resample``: every volume is first
    resampled in-plane from its header's spacing to ``new_spacing`` (y, x; default 1.4 x 1.4 mm), as the reference's readers do.

    Brain volumes (``downsample_steps=K``, optionally ``thick_slices=MM``): what the reference loads from its blurred files
    (datasets/common_brains.py:136-144, 206-208) made on the device -- one upload, one ``aesr_thick_slices(z_step=K)`` (skipped when
    ``thick_slices`` is None: the files are blurred already, only ``[::K]`` applies) and one min / max rescale (``percs`` must be
    (0, 100)).  The result is a list of CUDA tensors [ceil(Z / K), H, W], which ``BrainTripletAugmenter`` uses as its cache as they are."""
    import os
    from . import volume_io
    brain = _check_brain_options(thick_slices, downsample_steps, resample)
    if brain and tuple(percs) != (0, 100):
        raise NotImplementedError("percs=%r: only the brain loaders' default window (0, 100), i.e. min / max, is built on the device" % (percs,))
    vols = []
    for name in sorted(os.listdir(path)):
        f = os.path.join(path, name)
        low = name.lower()
        spacing = None
        if low.endswith(".npy"):
            arr = np.load(f)
        elif low.endswith((".nii", ".nii.gz", ".mha", ".mhd")):
            v = volume_io.read_volume(f)
            arr, spacing = v.array, tuple(v.spacing[:3][::-1])
        else:
            continue
        if resample:
            arr = _resample_to(arr, spacing, new_spacing, f)
        frames = [arr] if arr.ndim == 3 else list(arr)
        for v in frames:
            v = np.asarray(v, dtype=np.float32)
            if v.ndim != 3:
                raise ValueError("%s: expected a 3-D or 4-D volume, got shape %s" % (f, arr.shape))
            if brain:
                from .datasets.common_brains import lr_volume_on_device
                vols.append(lr_volume_on_device(v, thick_slices, downsample_steps, device=device))
                continue
            vols.append(v if (v.min() >= 0 and v.max() <= 1) else rescale_intensities(v))
    if not vols:
        raise FileNotFoundError("no .npy / .nii / .mha / .mhd volumes in %s" % path)
    return vols


load_volumes = load_volume_dir


def load_image_dict(path, max_patients=2, resample=False, new_spacing=None, thick_slices=None, downsample_steps=None, include_hr=True,
                    device="cuda"):
    """The in-memory validation images ``validate(image_dict=...)`` previews (train_cardiac_aesr.py:49-53 of the reference: two 4-D
    patients): {p_id: {'image': [t,z,y,x] float32 in [0,1], 'patient_id': 'patientNNN', 'spacing': (z,y,x)}} from the first
    ``max_patients`` volumes of a directory (a 3-D volume counts as one frame).  p_id: the digits in the file name, else its rank.
    ``resample``: resample in-plane to ``new_spacing`` (default 1.4 x 1.4 mm) before the intensities are rescaled; 'spacing' then
    reports [z, new_y, new_x] and 'original_spacing' keeps the file's own, as the reference's ``preprocessed4d`` does.

    Brain volumes (``downsample_steps=K``, optionally ``thick_slices=MM``; 3-D files only): the LR / HR evaluation pair of the
    reference's ``get_images(..., do_downsample=True, include_hr_images=True)``.  'image' is [ceil(Z / K), y, x]: the volume blurred on
    the device (skipped when ``thick_slices`` is None), sub-sampled and rescaled to [0, 1] by its min / max; 'image_hr' (with
    ``include_hr``) is the file's own array as float32, untouched, which ``evaluate`` scores against; 'spacing' is the file's, and
    'num_slices' counts the slices of 'image'."""
    import os
    import re
    from . import volume_io
    brain = _check_brain_options(thick_slices, downsample_steps, resample)
    out = {}
    for rank, name in enumerate(sorted(os.listdir(path))):
        f, low = os.path.join(path, name), name.lower()
        if low.endswith(".npy"):
            arr, spacing = np.load(f), (1.0, 1.0, 1.0)
        elif low.endswith((".nii", ".nii.gz", ".mha", ".mhd")):
            v = volume_io.read_volume(f)
            arr, spacing = v.array, tuple(v.spacing[:3][::-1])
        else:
            continue
        original_spacing = spacing
        if brain:
            from .datasets.common_brains import lr_volume_on_device
            hr = np.asarray(arr, dtype=np.float32)
            if hr.ndim != 3:
                raise ValueError("%s: a brain volume is 3-D [z, y, x], got shape %s" % (f, hr.shape))
            lr = lr_volume_on_device(hr, thick_slices, downsample_steps, device=device).cpu().numpy()
            digits = re.findall(r"\d+", name)
            p_id = int(digits[0]) if digits and int(digits[0]) not in out else 1000 + rank
            out[p_id] = {"image": lr, "image_hr": hr if include_hr else None, "patient_id": "patient{:03d}".format(p_id),
                         "spacing": np.asarray(spacing, dtype=np.float64), "num_slices": lr.shape[0]}
            if len(out) >= int(max_patients):
                break
            continue
        if resample:
            arr = _resample_to(arr, None if low.endswith(".npy") else spacing, new_spacing, f)
            ns = NEW_SPACING if new_spacing is None else tuple(new_spacing)[-2:]
            spacing = (spacing[0], float(ns[0]), float(ns[1]))
        arr = np.asarray(arr, dtype=np.float32)
        arr = arr[None] if arr.ndim == 3 else arr
        if arr.ndim != 4:
            raise ValueError("%s: expected a 3-D or 4-D image, got shape %s" % (f, arr.shape))
        if not (arr.min() >= 0 and arr.max() <= 1):
            arr = np.stack([rescale_intensities(a) for a in arr])
        digits = re.findall(r"\d+", name)
        p_id = int(digits[0]) if digits and int(digits[0]) not in out else 1000 + rank
        out[p_id] = {"image": arr, "patient_id": "patient{:03d}".format(p_id), "spacing": np.asarray(spacing, dtype=np.float64)}
        if resample:
            out[p_id]["original_spacing"] = np.asarray(original_spacing, dtype=np.float64)
        if len(out) >= int(max_patients):
            break
    if not out:
        raise FileNotFoundError("no .npy / .nii / .mha / .mhd images in %s" % path)
    return out


class TripletAugmenter:
    """``volumes``: list of float32 arrays [Z,H,W] already intensity-normalised to [0,1] (one per patient / frame)."""

    def __init__(self, volumes, width, aug_patch_size, rs=None, device="cuda"):
        self.width, self.aug = int(width), int(aug_patch_size)
        self.rs = rs if rs is not None else np.random.RandomState(1234)
        self.device = device
        offs, flat, self.shapes = [], [], []
        n = 0
        for v in volumes:
            v = np.ascontiguousarray(v, dtype=np.float32)
            if v.ndim != 3:
                raise ValueError("every volume must be [Z,H,W], got %s" % (v.shape,))
            offs.append(n)
            self.shapes.append(v.shape)
            flat.append(v.reshape(-1))
            n += v.size
        self.offsets = offs
        self.cache = torch.from_numpy(np.concatenate(flat)).to(device)        # the device-resident volume cache
        self._out = {}          # B -> (joined [3B,1,W,W] output buffer, alpha_from, alpha_to): reused by every batch of that size

    # ---- host-side random draws, in the reference's order ---------------------------------------------------------
    def _geometry(self, H, W):
        """Offset of the centre-cropped, padded image inside the source slice, and its size (shared_transforms.py:297-447)."""
        aug = self.aug
        dl_y = (aug - H) // 2 if H < aug else 0
        dl_x = (aug - W) // 2 if W < aug else 0
        Hp, Wp = max(H, aug), max(W, aug)
        half = int(aug / 2)
        sy, sx = int(Hp / 2) - half, int(Wp / 2) - half
        return sy - dl_y, sx - dl_x, 2 * half, 2 * half

    def draw_triplet(self, vol_id, slice_id, step=1):
        """Slice choice of the dataset's __getitem__ (data4d_simple.py:191-203): a random neighbour, the slice in between and
        a random from/to order.  With step == 1 the in-between slice is the neighbour itself in the reference; callers that
        train on sub-sampled volumes pass step = 2."""
        Z = self.shapes[vol_id][0]
        other = get_random_adjacent_slice(slice_id, Z, self.rs, step)
        between = (slice_id + other) // 2
        if int(self.rs.randint(0, 2)) == 0:            # == rs.choice([0, 1]), see get_random_adjacent_slice
            return slice_id, other, between
        return other, slice_id, between

    def draw_transform(self, vol_id):
        """[top, left] (only when a crop happens), gain, cutoff, k: shared_transforms.py:90-91, 376-377, 235."""
        _, H, W = self.shapes[vol_id]
        oy, ox, h, w = self._geometry(H, W)
        top = left = 0
        if not (h == self.width and w == self.width):
            top = int(self.rs.randint(0, h - self.width))
            left = int(self.rs.randint(0, w - self.width))
        gain = float(self.rs.uniform(2.5, 7.5))
        cutoff = float(self.rs.uniform(0.25, 0.75))
        k = int(self.rs.randint(0, 4))
        return oy + top, ox + left, gain, cutoff, k

    # ---- device side ------------------------------------------------------------------------------------------------
    def assemble(self, triplets, transforms=None, reuse_output=False):
        """triplets: list of (vol_id, z_from, z_to, z_between); transforms: list of (oy, ox, gain, cutoff, k) or None (drawn
        now, one sample after the other).  Returns {'image': [2B,1,W,W], 'slice_between': [B,1,W,W], 'alpha_from', 'alpha_to'}."""
        B, Wd = len(triplets), self.width
        if transforms is None:
            transforms = [self.draw_transform(t[0]) for t in triplets]
        if reuse_output:
            # ONE buffer [image | slice_between] per batch size, written again by every batch: the trainer's captured step reads its
            # inputs from exactly these addresses (AEBaseTrainer._train_graphed adopts "_persistent" batches as its static inputs), so
            # a training step costs the assemble launch and the graph replay -- no allocation, no fill, no copy of the batch
            if B not in self._out:
                both = torch.empty((3 * B, 1, Wd, Wd), device=self.device, dtype=torch.float32)
                half = torch.full((B, 1), 0.5, device=self.device, dtype=torch.float32)
                self._out[B] = (both, half, half.clone())
            both, a_from, a_to = self._out[B]
            image, between = both[:2 * B], both[2 * B:]
        else:
            image = torch.empty((2 * B, 1, Wd, Wd), device=self.device, dtype=torch.float32)
            between = torch.empty((B, 1, Wd, Wd), device=self.device, dtype=torch.float32)
        _hip.require_gpu_tensor(self.cache, "volume cache")
        for b0 in range(0, B, 64):
            n = min(64, B - b0)
            descs = (_hip.TripletDesc * n)()
            for i in range(n):
                vid, zf, zt, zb = triplets[b0 + i]
                oy, ox, gain, cutoff, k = transforms[b0 + i]
                Z, H, W = self.shapes[vid]
                if not (0 <= zf < Z and 0 <= zt < Z and 0 <= zb < Z):
                    raise ValueError("slice index outside volume %d (Z=%d)" % (vid, Z))
                descs[i] = _hip.TripletDesc(self.offsets[vid], H, W, zf, zt, zb, oy, ox, k, gain, cutoff)
            if B <= 64:
                img_dst, btw_dst = image, between
            else:       # more than one launch: each launch owns a contiguous [from | to] pair block -> assemble then scatter
                img_dst = torch.empty((2 * n, 1, Wd, Wd), device=self.device, dtype=torch.float32)
                btw_dst = between[b0:b0 + n]
            check(lib.aesr_triplet_assemble(ptr(self.cache), descs, n, Wd, ptr(img_dst), ptr(btw_dst), stream()),
                  "aesr_triplet_assemble")
            if B > 64:
                image[b0:b0 + n] = img_dst[:n]
                image[B + b0:B + b0 + n] = img_dst[n:]
        if reuse_output:
            return {"image": image, "slice_between": between, "alpha_from": a_from, "alpha_to": a_to, "_persistent": True}
        half = torch.full((B, 1), 0.5, device=self.device, dtype=torch.float32)
        return {"image": image, "slice_between": between, "alpha_from": half, "alpha_to": half.clone()}

    def next_batch(self, B, step=2, reuse_output=False, shard=None):
        """A random training batch: B random (volume, slice) pairs, neighbours ``step`` apart.  ``reuse_output``: the batch is written
        into this augmenter's persistent output buffer (valid until the next call) -- what the training loop uses.  ``shard`` = (rank,
        world): data parallel -- EVERY random number of the global batch is drawn (all ranks keep the same stream position and see the
        batch a single process would see), but only this rank's triplets [B r / W, B (r + 1) / W) are assembled: the host cost of a
        rank is the global batch's draws plus its own few descriptors, the device cost one launch over its own triplets."""
        trips = []
        for _ in range(B):
            vid = int(self.rs.randint(0, len(self.shapes)))
            Z = self.shapes[vid][0]
            if Z < step + 1:
                raise ValueError("volume %d has too few slices (%d) for step %d" % (vid, Z, step))
            sid = int(self.rs.randint(0, Z))
            zf, zt, zb = self.draw_triplet(vid, sid, step)
            trips.append((vid, zf, zt, zb))
        if shard is None:
            return self.assemble(trips, reuse_output=reuse_output)
        rank, world = int(shard[0]), int(shard[1])
        transforms = [self.draw_transform(t[0]) for t in trips]         # the order assemble() draws them in
        lo, hi = (B * rank) // world, (B * (rank + 1)) // world
        return self.assemble(trips[lo:hi], transforms[lo:hi], reuse_output=reuse_output)


# ---- brain volumes (datasets/common_brains.py, OASIS/dataset.py, dHCP/dataset.py of the reference) ---------------------------------
class BrainSampler:
    """The random draws of the reference's ``BrainDataset.__getitem__`` (datasets/common_brains.py:241-283), host only: from one
    (slice id, number of slices) the neighbour ``slice step`` away, the slice in between, the from / to order and the mixing
    coefficients, drawn from this sampler's own ``RandomState`` with the reference's calls in the reference's order.

    ``dataset``: 'OASIS' always regularises on neighbours 2 apart (OASIS/dataset.py:95-101: ``adjacent_plus`` -> 2, ``mix`` ->
    ``rs.choice([1, 2])``); every other brain dataset (dHCP, ADNI: the base class) uses ``downsample_steps``.

    ``adjacent``, and ``mix`` whenever it draws step 1, make the reference call ``rs.choice`` on the empty range between two
    neighbouring slices, which raises there; here that is a ``ValueError`` that says so."""

    def __init__(self, dataset, slice_selection="adjacent_plus", downsample_steps=1, rs=None):
        if slice_selection not in ("adjacent", "adjacent_plus", "mix"):
            raise ValueError("slice_selection=%r: one of 'adjacent', 'adjacent_plus', 'mix'" % (slice_selection,))
        self.dataset, self.slice_selection, self.downsample_steps = dataset, slice_selection, int(downsample_steps)
        self.rs = rs if rs is not None else np.random.RandomState(1234)

    def slice_step(self):
        plus = 2 if self.dataset == "OASIS" else self.downsample_steps
        if self.slice_selection == "adjacent":
            return 1
        if self.slice_selection == "adjacent_plus":
            return plus
        return int(self.rs.choice([1, plus]))

    def draw(self, slice_id, num_slices):
        """-> (slice_from, slice_to, slice_between, alpha_from, alpha_to); the alphas are float32, as the dataset stores them."""
        from .datasets.common_brains import determine_interpol_coefficients
        slice_id, num_slices = int(slice_id), int(num_slices)
        step = self.slice_step()
        last = num_slices - 1
        if slice_id + step > last:                      # datasets/common.py:34-43, with its rs.choice
            other = slice_id - step
        elif slice_id == 0:
            other = step
        elif slice_id - step < 0:
            other = slice_id + step
        else:
            other = int(self.rs.choice([slice_id - step, slice_id + step]))
        if not 0 <= other <= last:
            # fewer than 2 * step slices: the reference's rule leaves the volume here (and numpy wraps its -1 to the last slice)
            raise ValueError("slice %d of a volume of %d slices has no neighbour %d slices away (the volume needs at least %d slices)"
                             % (slice_id, num_slices, step, 2 * step))
        lo, hi = min(slice_id, other), max(slice_id, other)
        if hi - lo < 2:
            raise ValueError("slice_selection=%r drew slice step %d: there is no slice between %d and %d, and the reference raises here "
                             "too (rs.choice of an empty range, datasets/common_brains.py:281); use 'adjacent_plus'"
                             % (self.slice_selection, step, lo, hi))
        between = int(self.rs.choice(np.arange(lo + 1, hi)))
        if self.rs.choice([0, 1]) == 0:
            s_from, s_to = slice_id, other
        else:
            s_from, s_to = other, slice_id
        a_from, a_to = determine_interpol_coefficients(s_from, s_to, between)
        return s_from, s_to, between, np.float32(a_from), np.float32(a_to)


class BrainTripletAugmenter:
    """``TripletAugmenter`` for brain volumes: the batches of the reference's ``BrainDataset`` + ``get_transforms_brain`` +
    ``prepare_batch_pairs`` from a device-resident cache, one launch per batch.

    ``volumes``: [Z,H,W] float32 arrays or CUDA tensors in [0, 1] (``load_volume_dir(..., downsample_steps=K)`` returns such tensors;
    they are used as they are).  Differences from the cardiac class, all the reference's:
      - slices and coefficients come from a ``BrainSampler`` (``rs``); ``alpha_from`` / ``alpha_to`` vary per sample;
      - the transform numbers come from a SECOND ``RandomState`` (``rs_transform``: the reference's dataset and transforms hold two
        distinct default objects) in the brain order: crop top / left (only when a crop happens), then ``k``, then ``gain``, ``cutoff``;
      - geometry (datasets/common_brains.py:47-100): with ``width < aug_patch_size`` (the reference's 220 for OASIS, 256 for dHCP / ADNI)
        OASIS / ADNI slices are zero-padded up to ``aug_patch_size`` (``AdjustToPatchSize`` only pads) and a ``width`` window is cropped at
        random; dHCP slices are not padded.  A slice that is ``width`` x ``width`` already is not cropped and draws nothing.  Otherwise
        (no crop) OASIS / ADNI slices are padded up to ``width``, dHCP slices stay.  There is no centre crop: a slice that cannot be
        cropped, is larger than the patch without a crop, or is not ``width`` x ``width`` in the end is refused with a ``ValueError``;
      - ``raw=True``: the test transform (padding only, no rotation, no intensity curve) through ``aesr_triplet_assemble_raw``."""

    def __init__(self, volumes, width, aug_patch_size=None, dataset="OASIS", slice_selection="adjacent_plus", downsample_steps=1, rs=None,
                 rs_transform=None, device="cuda"):
        self.width = int(width)
        self.aug = int(aug_patch_size) if aug_patch_size else self.width
        self.dataset, self.device = dataset, device
        self.rs = rs if rs is not None else np.random.RandomState(1234)
        self.rs_transform = rs_transform if rs_transform is not None else np.random.RandomState(1234)
        self.sampler = BrainSampler(dataset, slice_selection, downsample_steps, self.rs)
        self.pads = dataset != "dHCP"
        self.crops = self.width < self.aug
        offs, flat, self.shapes = [], [], []
        n = 0
        for v in volumes:
            v = v.to(device=device, dtype=torch.float32) if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(device)
            if v.dim() != 3:
                raise ValueError("every volume must be [Z,H,W], got %s" % (tuple(v.shape),))
            offs.append(n)
            self.shapes.append(tuple(int(s) for s in v.shape))
            flat.append(v.reshape(-1))
            n += v.numel()
        self.offsets = offs
        step = 2 if dataset == "OASIS" else int(downsample_steps)
        short = [i for i, sh in enumerate(self.shapes) if sh[0] < 2 * step]
        if slice_selection != "adjacent" and short:
            raise ValueError("volume %d has %d slices: neighbours %d slices apart need at least %d (below that the reference's neighbour rule "
                             "leaves the volume)" % (short[0], self.shapes[short[0]][0], step, 2 * step))
        self.cache = flat[0].contiguous() if len(flat) == 1 else torch.cat(flat)        # the device-resident volume cache
        self._out = {}          # B -> (joined [3B,1,W,W] output buffer, alpha_from [B,1], alpha_to [B,1]): reused by every batch of that size
        self._host_alphas = {}  # B -> (pinned [2,B,1] staging of the coefficients, event recorded after its copy)

    # ---- host side ------------------------------------------------------------------------------------------------------------------
    def _padded(self, vol_id, target, pads=None):
        """(pad_top, pad_left, height, width) of a slice after ``AdjustToPatchSize((target, target))`` (shared_transforms.py:389-447)."""
        _, H, W = self.shapes[vol_id]
        if not (self.pads if pads is None else pads):
            return 0, 0, H, W
        return max(0, target - H) // 2, max(0, target - W) // 2, max(H, target), max(W, target)

    def draw_transform(self, vol_id):
        """(oy, ox, gain, cutoff, k), drawn from ``rs_transform``: [top, left] (only when a crop happens), k, gain, cutoff."""
        rs, wd = self.rs_transform, self.width
        pt, pl, h, w = self._padded(vol_id, self.aug if self.crops else wd)
        top = left = 0
        if self.crops and not (h == wd and w == wd):
            if h <= wd or w <= wd:
                raise ValueError("volume %d: a %d x %d slice cannot be cropped to %d x %d (RandomCrop draws from an empty range)"
                                 % (vol_id, h, w, wd, wd))
            top = int(rs.randint(0, h - wd))
            left = int(rs.randint(0, w - wd))
        elif not (h == wd and w == wd):
            raise ValueError("volume %d: slices are %d x %d after padding, not %d x %d, and no crop is configured (width < aug_patch_size)"
                             % (vol_id, h, w, wd, wd))
        k = int(rs.randint(0, 4))
        gain = float(rs.uniform(2.5, 7.5))
        cutoff = float(rs.uniform(0.25, 0.75))
        return top - pt, left - pl, gain, cutoff, k

    def test_transform(self, vol_id, size=None):
        """The test transform: padding up to ``width`` (OASIS / ADNI) or nothing (dHCP); no draw.  ``size``: every dataset's slices are
        padded up to size x size instead (``eval_size``)."""
        wd = self.width if size is None else int(size)
        pt, pl, h, w = self._padded(vol_id, wd, pads=None if size is None else True)
        if not (h == wd and w == wd):
            raise ValueError("volume %d: slices are %d x %d after padding, not %d x %d: the test transform does not crop"
                             % (vol_id, h, w, wd, wd))
        return -pt, -pl, 0.0, 0.0, 0

    def eval_size(self, multiple=1):
        """The smallest square the test transform can pad EVERY volume's slices to: >= ``width`` and every H, W, a multiple of
        ``multiple`` (the network's stride).  The reference's test transform leaves slices larger than the patch as they are (the
        network is convolutional) and its loader needs them equal-sized; one padded square serves volumes of unequal size."""
        s = max([self.width] + [max(H, W) for _, H, W in self.shapes])
        m = max(1, int(multiple))
        return (s + m - 1) // m * m

    # ---- device side ----------------------------------------------------------------------------------------------------------------
    def assemble(self, triplets, alphas, transforms=None, reuse_output=False, raw=False, size=None):
        """triplets: list of (vol_id, z_from, z_to, z_between); alphas: list of (alpha_from, alpha_to); transforms: list of
        (oy, ox, gain, cutoff, k) or None (drawn now, one sample after the other; ``raw``: the test transform, nothing drawn).
        Returns {'image': [2B,1,W,W], 'slice_between': [B,1,W,W], 'alpha_from': [B,1], 'alpha_to': [B,1]}.  ``reuse_output``: all four
        are this augmenter's persistent tensors of that batch size, written in place -- the coefficients too, so that a captured step
        reads the new ones.  ``size`` (with ``raw`` only): the slices are padded up to size x size instead of ``width``."""
        B, Wd = len(triplets), self.width
        if size is not None:
            if not raw or reuse_output:
                raise ValueError("size= goes with raw=True (the test transform) and tensors of its own")
            Wd = int(size)
        if len(alphas) != B:
            raise ValueError("%d triplets but %d coefficient pairs" % (B, len(alphas)))
        if transforms is None:
            transforms = [self.test_transform(t[0], size) if raw else self.draw_transform(t[0]) for t in triplets]
        if reuse_output:
            if B not in self._out:
                both = torch.empty((3 * B, 1, Wd, Wd), device=self.device, dtype=torch.float32)
                ab = torch.empty((2, B, 1), device=self.device, dtype=torch.float32)
                self._out[B] = (both, ab)
                self._host_alphas[B] = (torch.empty((2, B, 1), dtype=torch.float32).pin_memory(), torch.cuda.Event())
            both, ab = self._out[B]
            image, between = both[:2 * B], both[2 * B:]
            host, copied = self._host_alphas[B]
            copied.synchronize()            # the previous batch's copy has read the staging buffer (long done: no wait in practice)
        else:
            image = torch.empty((2 * B, 1, Wd, Wd), device=self.device, dtype=torch.float32)
            between = torch.empty((B, 1, Wd, Wd), device=self.device, dtype=torch.float32)
            ab = torch.empty((2, B, 1), device=self.device, dtype=torch.float32)
            host, copied = torch.empty((2, B, 1), dtype=torch.float32), None
        host[:, :, 0] = torch.from_numpy(np.asarray(alphas, dtype=np.float32).reshape(B, 2).T.copy())
        ab.copy_(host, non_blocking=copied is not None)
        if copied is not None:
            copied.record()
        launch = lib.aesr_triplet_assemble_raw if raw else lib.aesr_triplet_assemble
        _hip.require_gpu_tensor(self.cache, "volume cache")
        for b0 in range(0, B, 64):
            n = min(64, B - b0)
            descs = (_hip.TripletDesc * n)()
            for i in range(n):
                vid, zf, zt, zb = triplets[b0 + i]
                oy, ox, gain, cutoff, k = transforms[b0 + i]
                Z, H, W = self.shapes[vid]
                if not (0 <= zf < Z and 0 <= zt < Z and 0 <= zb < Z):
                    raise ValueError("slice index outside volume %d (Z=%d)" % (vid, Z))
                descs[i] = _hip.TripletDesc(self.offsets[vid], H, W, zf, zt, zb, oy, ox, k, gain, cutoff)
            if B <= 64:
                img_dst, btw_dst = image, between
            else:       # more than one launch: each launch owns a contiguous [from | to] pair block -> assemble then scatter
                img_dst = torch.empty((2 * n, 1, Wd, Wd), device=self.device, dtype=torch.float32)
                btw_dst = between[b0:b0 + n]
            check(launch(ptr(self.cache), descs, n, Wd, ptr(img_dst), ptr(btw_dst), stream()),
                  "aesr_triplet_assemble_raw" if raw else "aesr_triplet_assemble")
            if B > 64:
                image[b0:b0 + n] = img_dst[:n]
                image[B + b0:B + b0 + n] = img_dst[n:]
        out = {"image": image, "slice_between": between, "alpha_from": ab[0], "alpha_to": ab[1]}
        if reuse_output:
            out["_persistent"] = True
        return out

    def next_batch(self, B, reuse_output=False, shard=None, raw=False, size=None):
        """A random batch: B random (volume, slice) pairs, each completed by the sampler.  ``reuse_output`` and ``shard`` = (rank, world)
        as in ``TripletAugmenter.next_batch``: every rank draws the whole global batch (slices from ``rs``, then transforms from
        ``rs_transform``) and assembles its own triplets [B r / W, B (r + 1) / W)."""
        trips, alphas = [], []
        for _ in range(B):
            vid = int(self.rs.randint(0, len(self.shapes)))
            Z = self.shapes[vid][0]
            sid = int(self.rs.randint(0, Z))
            zf, zt, zb, af, at = self.sampler.draw(sid, Z)
            trips.append((vid, zf, zt, zb))
            alphas.append((af, at))
        transforms = [self.test_transform(t[0], size) if raw else self.draw_transform(t[0]) for t in trips]
        lo, hi = 0, B
        if shard is not None:
            rank, world = int(shard[0]), int(shard[1])
            lo, hi = (B * rank) // world, (B * (rank + 1)) // world
        return self.assemble(trips[lo:hi], alphas[lo:hi], transforms[lo:hi], reuse_output=reuse_output, raw=raw, size=size)


# ---- labelled cardiac volumes (datasets/ACDC/data_with_labels.py of the reference) ---------------------------------------------------
_VOLUME_EXTENSIONS = (".nii.gz", ".npy", ".nii", ".mha", ".mhd")


def _volume_files(path):
    """{stem: file name} of the volume files of a directory (the stem is the name without its extension, case kept)."""
    import os
    out = {}
    for name in sorted(os.listdir(path)):
        ext = next((e for e in _VOLUME_EXTENSIONS if name.lower().endswith(e)), None)
        if ext is None:
            continue
        stem = name[:-len(ext)]
        if stem in out:
            raise ValueError("%s: %s and %s share the stem %r, so a label file cannot be paired by name" % (path, out[stem], name, stem))
        out[stem] = name
    return out


def _read_volume_file(f):
    """(array, spacing (z, y, x) or None for a .npy file)"""
    from . import volume_io
    if f.lower().endswith(".npy"):
        return np.load(f), None
    v = volume_io.read_volume(f)
    return v.array, tuple(v.spacing[:3][::-1])


def _as_label_bytes(lab, what):
    """A label array as uint8; ValueError (naming ``what``) unless every value is an integer in 0 ... 255."""
    lab = np.asarray(lab)
    if lab.dtype != np.uint8:
        if lab.dtype == bool or not np.issubdtype(lab.dtype, np.number) or np.iscomplexobj(lab):
            raise ValueError("%s: labels must be numbers, got dtype %s" % (what, lab.dtype))
        if lab.size and not np.all(np.isfinite(lab)):
            raise ValueError("%s: labels must be finite" % what)
        if lab.size and not np.array_equal(lab, np.round(lab)):
            raise ValueError("%s: labels must be integral (class ids), found %r" % (what, float(lab[lab != np.round(lab)].flat[0])))
        if lab.size and (lab.min() < 0 or lab.max() > 255):
            raise ValueError("%s: labels must lie within 0 ... 255 (they are cached as bytes), found %r ... %r" % (what, lab.min(), lab.max()))
    return np.ascontiguousarray(lab, dtype=np.uint8)


def load_labelled_volume_dir(images_dir, labels_dir, resample=False, new_spacing=None):
    """(volumes, labels) for ``LabelledTripletAugmenter``: the image files of ``images_dir`` (as ``load_volume_dir`` reads and rescales them;
    4-D files give one volume per frame) and, paired BY NAME, the label maps of ``labels_dir`` -- the same stem, any supported extension
    (``vol0.nii.gz`` pairs with ``vol0.npy``).  An image without a label file, or a label file without an image, is a ``FileNotFoundError``.
    Labels must be integral, within 0 ... 255 and of their image's shape (``ValueError`` naming the file); they come back as uint8.

    ``resample``: images go through ``load_volume_dir``'s in-plane resampling (blur, linear) and labels through
    ``apply_2d_zoom_3d(order=0, do_blur=False, as_type=int)`` -- nearest sample, never a mixture of class ids -- as the reference's
    ``ACDCImage`` does; both from the IMAGE file's spacing, so the two keep one shape."""
    volumes, labels = [], []
    for f, lf in _paired_volume_files(images_dir, labels_dir):
        arr, lab, _ = _read_labelled_pair(f, lf, resample, new_spacing)
        for v, l in zip([arr] if arr.ndim == 3 else list(arr), [lab] if lab.ndim == 3 else list(lab)):
            v = np.asarray(v, dtype=np.float32)
            volumes.append(v if (v.min() >= 0 and v.max() <= 1) else rescale_intensities(v))
            labels.append(np.ascontiguousarray(l))
    return volumes, labels


def _paired_volume_files(images_dir, labels_dir):
    """[(image file, label file)] of two directories paired by stem, in the order of the sorted stems; an empty image directory, an image
    without a label file or a label file without an image is a ``FileNotFoundError``."""
    import os
    imgs, labs = _volume_files(images_dir), _volume_files(labels_dir)
    if not imgs:
        raise FileNotFoundError("no .npy / .nii / .mha / .mhd volumes in %s" % images_dir)
    for stem in imgs:
        if stem not in labs:
            raise FileNotFoundError("%s has no label file %s.* in %s" % (os.path.join(images_dir, imgs[stem]), stem, labels_dir))
    for stem in labs:
        if stem not in imgs:
            raise FileNotFoundError("%s has no image file %s.* in %s" % (os.path.join(labels_dir, labs[stem]), stem, images_dir))
    return [(os.path.join(images_dir, imgs[stem]), os.path.join(labels_dir, labs[stem])) for stem in sorted(imgs)]


def _read_labelled_pair(f, lf, resample, new_spacing):
    """(image array, labels uint8, the image file's spacing (z, y, x) or None) of one image / label file pair, 3-D or 4-D, shapes equal,
    labels integral within 0 ... 255 (``ValueError`` naming the file); ``resample``: both resampled in-plane from the IMAGE file's spacing,
    the image with blur and linear interpolation, the labels by nearest sample.  Intensities are not rescaled here."""
    from .datasets.common import apply_2d_zoom_3d, apply_2d_zoom_4d
    arr, spacing = _read_volume_file(f)
    lab, _ = _read_volume_file(lf)
    if arr.ndim not in (3, 4):
        raise ValueError("%s: expected a 3-D or 4-D volume, got shape %s" % (f, arr.shape))
    if tuple(lab.shape) != tuple(arr.shape):
        raise ValueError("%s: the label map's shape %s is not its image's %s (%s)" % (lf, tuple(lab.shape), tuple(arr.shape), f))
    lab = _as_label_bytes(lab, lf)
    if resample:
        arr = _resample_to(arr, spacing, new_spacing, f)
        fn = apply_2d_zoom_3d if lab.ndim == 3 else apply_2d_zoom_4d
        lab = _as_label_bytes(fn(lab.astype(np.float32), spacing, NEW_SPACING if new_spacing is None else new_spacing, order=0,
                                 do_blur=False, as_type=int), lf)
        assert tuple(lab.shape) == tuple(arr.shape)
    return arr, lab, spacing


def load_labelled_image_dict(images_dir, labels_dir, max_patients=2, resample=False, new_spacing=None):
    """The in-memory validation patients of the multi-channel trainers' ``validate(image_dict=...)``: ``load_image_dict`` for images that
    come with label maps.  {p_id: {'image': [t,z,y,x] float32 in [0,1], 'labels': [t,z,y,x] uint8, 'patient_id': 'patientNNN',
    'spacing': (z,y,x)[, 'original_spacing']}} from the first ``max_patients`` image files (sorted by stem) of ``images_dir`` and the label
    files of ``labels_dir``, paired by stem exactly as ``load_labelled_volume_dir`` pairs them, with its checks and its errors (both
    directories are checked for unpaired files as a whole; shapes and label values of the files that are read).  A 3-D file counts as one
    frame.  p_id: the digits in the image file's name, else its rank.  ``resample``: image and labels resampled in-plane to ``new_spacing``
    (labels by nearest sample) before the intensities are rescaled; 'spacing' then reports [z, new_y, new_x] and 'original_spacing' the
    file's own.  A .npy file carries no spacing: (1, 1, 1), and ``resample`` refuses it."""
    import os
    import re
    out = {}
    for rank, (f, lf) in enumerate(_paired_volume_files(images_dir, labels_dir)):
        if len(out) >= int(max_patients):
            break
        arr, lab, spacing = _read_labelled_pair(f, lf, resample, new_spacing)
        original_spacing = spacing = (1.0, 1.0, 1.0) if spacing is None else spacing
        if resample:
            ns = NEW_SPACING if new_spacing is None else tuple(new_spacing)[-2:]
            spacing = (spacing[0], float(ns[0]), float(ns[1]))
        arr = np.asarray(arr, dtype=np.float32)
        arr, lab = (arr[None], lab[None]) if arr.ndim == 3 else (arr, lab)
        if not (arr.min() >= 0 and arr.max() <= 1):
            arr = np.stack([rescale_intensities(a) for a in arr]).astype(np.float32)
        digits = re.findall(r"\d+", os.path.basename(f))
        p_id = int(digits[0]) if digits and int(digits[0]) not in out else 1000 + rank
        out[p_id] = {"image": arr, "labels": np.ascontiguousarray(lab), "patient_id": "patient{:03d}".format(p_id),
                     "spacing": np.asarray(spacing, dtype=np.float64)}
        if resample:
            out[p_id]["original_spacing"] = np.asarray(original_spacing, dtype=np.float64)
    return out


class LabelledTripletAugmenter(TripletAugmenter):
    """``TripletAugmenter`` for volumes that come with a label map: the batches of the reference's ``ACDCDatasetEDESPairs`` under the
    transforms of train_cardiac_aesr.py:83-105 and the 6-channel branch of ``prepare_batch_pairs``, from two flat device caches (float32
    images, uint8 labels; one offset addresses both) in one launch per batch (``aesr_labelled_triplet_assemble``,
    include/aesr_hip_labelprep.h).  ``image`` is [2B, 2, W, W] and ``slice_between`` [B, 2, W, W]: channel 0 the intensities, channel 1 the
    class ids as floats -- cropped and rotated together, the intensity curve on channel 0 only, padding 0 (background) in the labels.

    ``volumes`` / ``labels``: lists of [Z, H, W] arrays of equal shapes, intensities in [0, 1], labels integral in 0 ... 255
    (``load_labelled_volume_dir`` returns such a pair).  Differences from the cardiac class, all the reference's:
      - ``draw_sample`` follows ``ACDCDatasetEDESPairs.__getitem__``: the slice step by ``slice_selection`` ('adjacent' 1, 'adjacent_plus' 2,
        'mix' one draw), the neighbour, the slice in between -- ``(a + b) // 2`` when ``a + b`` is even, else the slice itself with
        ``is_inbetween = 0`` --, the from / to order, then the transform's numbers;
      - the transform's numbers come from ``rs_transform``, by default the SAME object as ``rs``: the training script hands one global
        RandomState to the dataset and to the transforms.  The draws themselves are ``TripletAugmenter.draw_transform``'s;
      - ``raw=True``: the script's test transform (``test_transform``), no draw, no intensity curve, no rotation.
    Not the reference's: a batch is B draws of (volume, slice) by ``rs.randint`` (the reference's loader shuffles with torch's generator);
    ``RandomAnyRotation`` (the dataset's own default transform, which the training script never uses) is not built."""

    def __init__(self, volumes, labels, width, aug_patch_size, slice_selection="adjacent_plus", rs=None, rs_transform=None, device="cuda"):
        if slice_selection not in ("adjacent", "adjacent_plus", "mix"):
            raise ValueError("slice_selection=%r: one of 'adjacent', 'adjacent_plus', 'mix'" % (slice_selection,))
        volumes, labels = list(volumes), list(labels)
        if len(volumes) != len(labels) or not volumes:
            raise ValueError("%d volumes but %d label maps" % (len(volumes), len(labels)))
        flat = []
        for i, (v, l) in enumerate(zip(volumes, labels)):
            if np.ndim(v) != 3 or tuple(np.shape(l)) != tuple(np.shape(v)):
                raise ValueError("volume %d: the image is %s and its label map %s; both must be one [Z,H,W]" % (i, np.shape(v), np.shape(l)))
            flat.append(_as_label_bytes(l, "label map %d" % i).reshape(-1))
            step = 1 if slice_selection == "adjacent" else 2
            if np.shape(v)[0] < 2 * step:
                raise ValueError("volume %d has %d slices: neighbours %d slices apart need at least %d (below that the reference's neighbour "
                                 "rule leaves the volume)" % (i, np.shape(v)[0], step, 2 * step))
        super().__init__(volumes, width, aug_patch_size, rs=rs, device=device)
        self.slice_selection = slice_selection
        self.rs_transform = rs_transform if rs_transform is not None else self.rs
        self.label_cache = torch.from_numpy(np.concatenate(flat)).to(device)        # uint8, the layout of self.cache
        assert self.label_cache.numel() == self.cache.numel()

    # ---- host side ------------------------------------------------------------------------------------------------------------------
    def draw_transform(self, vol_id):
        """``TripletAugmenter.draw_transform`` -- [top, left] (only when a crop happens), gain, cutoff, k -- drawn from ``rs_transform``."""
        rs, self.rs = self.rs, self.rs_transform          # the parent draws from self.rs: lend it the transforms' state for this call
        try:
            return super().draw_transform(vol_id)
        finally:
            self.rs = rs

    def test_size(self, size=None):
        """Width of a ``raw`` batch: ``CenterCrop`` keeps ``2 * int(canvas / 2)``; the canvas is ``aug_patch_size`` for ``width <= 128``,
        else ``width`` (train_cardiac_aesr.py:99-104), or ``size``."""
        canvas = int(size) if size is not None else (self.aug if self.width <= 128 else self.width)
        return 2 * int(canvas / 2)

    def test_transform(self, vol_id, size=None):
        """The script's ``transform_te``, no draw: for ``width <= 128`` a centre crop of ``aug_patch_size``, otherwise zero padding up to
        ``width`` and a centre crop of ``width``; ``size``: that canvas instead.  The reference's first branch does not pad, so a slice
        smaller than the crop leaves it with slices of unequal size (or, between the two sizes, wrapped indices); here it is padded with
        zeros as in the second branch -- for slices at least as large as the crop the two agree."""
        _, H, W = self.shapes[vol_id]
        aug = self.aug
        self.aug = int(size) if size is not None else (self.aug if self.width <= 128 else self.width)
        try:
            oy, ox, _, _ = self._geometry(H, W)
        finally:
            self.aug = aug
        return oy, ox, 0.0, 0.0, 0

    def draw_sample(self, vol_id, slice_id, raw=False):
        """``ACDCDatasetEDESPairs.__getitem__`` (datasets/ACDC/data_with_labels.py:141-155, 197-214) for one (volume, slice):
        -> ((vol_id, z_from, z_to, z_between), is_inbetween, (oy, ox, gain, cutoff, k))."""
        Z = self.shapes[vol_id][0]
        slice_id = int(slice_id)
        if not 0 <= slice_id < Z:
            raise ValueError("slice index outside volume %d (Z=%d)" % (vol_id, Z))
        if self.slice_selection == "adjacent":
            step = 1
        elif self.slice_selection == "adjacent_plus":
            step = 2
        else:
            step = (1, 2)[int(self.rs.randint(0, 2))]          # == rs.choice([1, 2]), see get_random_adjacent_slice
        other = int(get_random_adjacent_slice(slice_id, Z, self.rs, step))
        if (slice_id + other) % 2 == 0:
            between, is_inbetween = (slice_id + other) // 2, 1
        else:
            between, is_inbetween = slice_id, 0
        if int(self.rs.randint(0, 2)) == 0:            # == rs.choice([0, 1])
            z_from, z_to = slice_id, other
        else:
            z_from, z_to = other, slice_id
        transform = self.test_transform(vol_id) if raw else self.draw_transform(vol_id)
        return (vol_id, z_from, z_to, between), is_inbetween, transform

    # ---- device side ----------------------------------------------------------------------------------------------------------------
    def assemble(self, samples, transforms=None, reuse_output=False, raw=False, size=None):
        """samples: list of (vol_id, z_from, z_to, z_between); transforms: list of (oy, ox, gain, cutoff, k) or None (drawn now, one sample
        after the other; ``raw``: the test transform, nothing drawn).  Returns {'image': [2B,2,W,W], 'slice_between': [B,2,W,W],
        'alpha_from', 'alpha_to': [B,1] of 0.5, 'is_inbetween': [2B,1] (0 where the slice between is one of the pair, as the reference marks
        it), 'loss_mask': [2B,1] of ones}.  ``reuse_output``: image and slice_between are views of ONE persistent [3B,2,W,W] buffer of this
        augmenter, written again by every batch of that size.  ``size`` (with ``raw`` only): the test transform's canvas."""
        B, Wd = len(samples), self.width
        if size is not None and not raw:
            raise ValueError("size= goes with raw=True (the test transform)")
        if raw:
            Wd = self.test_size(size)
        if transforms is None:
            transforms = [self.test_transform(s[0], size) if raw else self.draw_transform(s[0]) for s in samples]
        if len(transforms) != B:
            raise ValueError("%d samples but %d transforms" % (B, len(transforms)))
        for vid, zf, zt, zb in samples:
            Z = self.shapes[vid][0]
            if not (0 <= zf < Z and 0 <= zt < Z and 0 <= zb < Z):
                raise ValueError("slice index outside volume %d (Z=%d)" % (vid, Z))
        inb = torch.tensor([[0.0 if s[3] in (s[1], s[2]) else 1.0] for s in samples] * 2, dtype=torch.float32).reshape(2 * B, 1)
        if reuse_output:
            key = (B, Wd)
            if key not in self._out:
                both = torch.empty((3 * B, 2, Wd, Wd), device=self.device, dtype=torch.float32)
                half = torch.full((B, 1), 0.5, device=self.device, dtype=torch.float32)
                self._out[key] = (both, half, half.clone(), torch.empty((2 * B, 1), device=self.device, dtype=torch.float32),
                                  torch.ones((2 * B, 1), device=self.device, dtype=torch.float32))
            both, a_from, a_to, inb_dev, ones = self._out[key]
            inb_dev.copy_(inb)
            image, between = both[:2 * B], both[2 * B:]
        else:
            image = torch.empty((2 * B, 2, Wd, Wd), device=self.device, dtype=torch.float32)
            between = torch.empty((B, 2, Wd, Wd), device=self.device, dtype=torch.float32)
            a_from = torch.full((B, 1), 0.5, device=self.device, dtype=torch.float32)
            a_to, inb_dev = a_from.clone(), inb.to(self.device)
            ones = torch.ones((2 * B, 1), device=self.device, dtype=torch.float32)
        launch = lib.aesr_labelled_triplet_assemble_raw if raw else lib.aesr_labelled_triplet_assemble
        _hip.require_gpu_tensor(self.cache, "volume cache")
        _hip.require_gpu_tensor(self.label_cache, "label cache", torch.uint8)
        for b0 in range(0, B, 64):
            n = min(64, B - b0)
            descs = (_hip.TripletDesc * n)()
            for i in range(n):
                vid, zf, zt, zb = samples[b0 + i]
                oy, ox, gain, cutoff, k = transforms[b0 + i]
                _, H, W = self.shapes[vid]
                descs[i] = _hip.TripletDesc(self.offsets[vid], H, W, zf, zt, zb, oy, ox, k, gain, cutoff)
            if B <= 64:
                img_dst, btw_dst = image, between
            else:       # more than one launch: each launch owns a contiguous [from | to] pair block -> assemble then scatter
                img_dst = torch.empty((2 * n, 2, Wd, Wd), device=self.device, dtype=torch.float32)
                btw_dst = between[b0:b0 + n]
            check(launch(ptr(self.cache), ptr(self.label_cache), descs, n, Wd, ptr(img_dst), ptr(btw_dst), stream()),
                  "aesr_labelled_triplet_assemble_raw" if raw else "aesr_labelled_triplet_assemble")
            if B > 64:
                image[b0:b0 + n] = img_dst[:n]
                image[B + b0:B + b0 + n] = img_dst[n:]
        out = {"image": image, "slice_between": between, "alpha_from": a_from, "alpha_to": a_to, "is_inbetween": inb_dev, "loss_mask": ones}
        if reuse_output:
            out["_persistent"] = True
        return out

    def next_batch(self, B, reuse_output=False, shard=None, raw=False):
        """A random batch: B random (volume, slice) pairs, each completed by ``draw_sample`` -- its slices, then its transform, sample after
        sample, which is the order one shared RandomState serves the reference's dataset and transforms in.  ``reuse_output`` and ``shard`` =
        (rank, world) as in ``TripletAugmenter.next_batch``: every rank draws the whole global batch and assembles its own samples
        [B r / W, B (r + 1) / W)."""
        samples, transforms = [], []
        for _ in range(B):
            vid = int(self.rs.randint(0, len(self.shapes)))
            sid = int(self.rs.randint(0, self.shapes[vid][0]))
            s, _, t = self.draw_sample(vid, sid, raw=raw)
            samples.append(s)
            transforms.append(t)
        lo, hi = 0, B
        if shard is not None:
            rank, world = int(shard[0]), int(shard[1])
            lo, hi = (B * rank) // world, (B * (rank + 1)) // world
        return self.assemble(samples[lo:hi], transforms[lo:hi], reuse_output=reuse_output, raw=raw)
