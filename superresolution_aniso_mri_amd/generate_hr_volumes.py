"""Slice-synthesis inference: the reference's ``generate_hr_volumes.py`` (:12-101 ``create_super_volume`` /
``latent_space_interp``, :104-183 I/O + ``main``) on the HIP engine.

The reference re-encodes both neighbour stacks for EVERY alpha (2n encoder passes per slice pair) and
copies every decoded stack to the host.  Here each slice is encoded ONCE (eval-mode BatchNorm makes results independent
of batch composition), the latents stay resident in HBM, the decoder's first convolution runs once per SLICE (it is linear: its
output for a latent mix is the mix of its outputs), all (z-1)*n mixes are formed on its pre-activations by ONE launch and the rest
of the decoder runs on them as ONE batch, the interleave and clamp happen on the device and there is a single device-to-host copy
at the end.
Conventions kept: ``alpha*enc(later slice) + (1-alpha)*enc(earlier slice)``, alphas = linspace(0,1,n+2)[1:-1],
output order [orig_0, interp_0(a_1..a_n), orig_1, ...], clamp to [0,1], new z-spacing = old/(n+1).

``--resample`` (the reference's ``CardiacImage(resample=True)`` on the way in, datasets/cardiac_image.py:80-88, and
``save_3d_volume(..., resample=True)`` on the way out, evaluate/create_HR_images.py:83-87): the volume is resampled in-plane to the
training spacing (``--new_spacing``, default 1.4 x 1.4 mm) BEFORE the percentile normalisation, synthesised, and resampled back to the
file's own in-plane spacing before it is written -- both resamplings on the device (datasets/common.py, csrc/inplane.hip), so the
volume crosses PCIe once each way.  Without the flag nothing changes.

``--method linear|bspline|lanczos|nearest`` writes a conventional through-plane baseline instead (the reference's
``create_simple_interpolation``, evaluate/common.py:74-118): no model is loaded, the volume is expanded along z by
``num_interpolations + 1`` on the device (evaluate/z_interp.py, csrc/z_expand.hip) with its intensities as they are, and written with the
z spacing divided by the same factor.  ``--align itk`` (default) is SimpleITK's ExpandImageFilter grid, ``--align grid`` the layout of the
model's output.

``--labels_input_dir DIR`` (a multi-channel model, ``--dataset ACDCLBL``): every image has a label volume of the same file name in DIR; the
label map goes through the network as the second channel and ``<name>_labels`` is written beside the super-resolved image -- the given
labels at the kept slots, in between the arg-max maps decoded from the same mixed latents as the in-between slices -- as an unsigned
8-bit volume with the image's new z spacing.  Such a model is refused without the flag.

``--target_spacing_z MM`` / ``--isotropic`` (instead of ``--num_interpolations``): slices MM apart -- or as far apart as the written
in-plane pixels -- on the grid of evaluate/z_grid.py: slice j at input coordinate j * MM / (the file's z spacing), the first slice the
first input slice, none beyond the last.  Input slices the grid hits are passed through; every other slice is the mix of its two
neighbours with its own alpha (``HipAE.decode_mixes_at``: one mixing launch per gap on the first convolution's pre-activations, one
decoder batch).  ``--method linear|nearest`` write their baseline on the same grid through evaluate/reslice.py.  The file is written
with z spacing MM and its origin and direction as they were; ``.npy`` volumes say their z spacing with ``--spacing_z``."""
import argparse
import os
from pathlib import Path

import numpy as np
import torch

from . import _hip, ops


def _encode(trainer, x):
    return trainer.encode(x, use_sr_model=True)


def latent_space_interp(alpha, trainer, img1, img2, device=None, with_labels=False):
    """One alpha: decode(alpha*enc(img1) + (1-alpha)*enc(img2)) (reference :72-101).  Returns CPU tensors.  ``with_labels``: the images
    carry their label maps as channel 1 (a multi-channel model); ``inter_label`` is the arg-max map decoded from the same mixed latent."""
    dev = device or trainer.args["device"]
    z = torch.cat([_encode(trainer, img1.float().to(dev)), _encode(trainer, img2.float().to(dev))], dim=0)
    inter = trainer.decode(ops.lerp_mix(z, float(alpha), float(1 - alpha)), use_sr_model=True)
    if with_labels:
        return {"inter_image": inter["image"].detach().cpu().contiguous(), "inter_label": inter["pred_labels"].detach().cpu()}
    _no_label_model(inter)
    return {"inter_image": inter.detach().cpu().contiguous(), "inter_label": None}


def _no_label_model(decoded):
    if isinstance(decoded, dict):
        raise ValueError("this is a multi-channel model (image + label map): it needs the label volume too (labels=... / with_labels=True, "
                         "generate_hr_volumes --labels_input_dir)")


def _interleave(orig, synth, n, clamp):
    """orig [Z, H, W], synth [n (Z - 1), H, W] (row k (Z - 1) + i) or None -> [(Z - 1)(n + 1) + 1, H, W]: slice i at slot i (n + 1), its n
    synthesised successors behind it; ``clamp`` = (lo, hi)."""
    Z, H, W = orig.shape
    if orig.is_cuda and (H * W) % 4 == 0:
        # interleave + clamp: one pass over the volume (a channel of a two-channel volume is gathered first)
        return ops.interleave_clamp(orig.contiguous(), synth, n, clamp[0], clamp[1])
    out = torch.empty(((Z - 1) * (n + 1) + 1, H, W), device=orig.device, dtype=torch.float32)
    out[::n + 1] = orig
    if synth is not None:
        synth = synth.reshape(n, Z - 1, H, W)
        for k in range(n):
            out[k + 1::n + 1] = synth[k]
    return out.clamp_(clamp[0], clamp[1])


def _assemble(kept, synth, grid, clamp):
    """kept [Z, H, W], synth [S, H, W] (the synthesised slices in ascending position) or None -> [grid.J, H, W]: every original slot of
    the grid takes the kept slice it is, every other slot the next synthesised slice; ``clamp`` = (lo, hi).  By index on the device."""
    out = torch.empty((grid.J,) + tuple(kept.shape[1:]), device=kept.device, dtype=torch.float32)
    slots = torch.from_numpy(np.flatnonzero(grid.is_original)).to(kept.device)
    out.index_copy_(0, slots, kept.float().index_select(0, torch.from_numpy(grid.source[grid.is_original]).to(kept.device)))
    if synth is not None:
        out.index_copy_(0, torch.from_numpy(np.flatnonzero(~grid.is_original)).to(kept.device), synth.float())
    return out.clamp_(clamp[0], clamp[1])


def _decode_on_grid(trainer, lat, grid):
    """The decoded synthesised slices of ``grid`` in ascending position: ``decode_mixes_at`` where the model has it, else per-slice
    coefficients on gathered latent pairs and one decode."""
    model = trainer._use_sr_model(True)
    model.eval()
    dec = model.decode_mixes_at(lat, grid.gap_alphas) if hasattr(model, "decode_mixes_at") else None
    if dec is None:
        synth = ~grid.is_original
        gap = torch.from_numpy(grid.gap[synth]).to(lat.device)
        zpair = torch.cat([lat.index_select(0, gap + 1), lat.index_select(0, gap)], dim=0)      # later slices, then earlier ones
        a = grid.alpha[synth]
        a_from, a_to = torch.from_numpy(a.astype(np.float32)), torch.from_numpy((1.0 - a).astype(np.float32))
        dec = trainer.decode(ops.lerp_mix(zpair, a_from.to(lat.device), a_to.to(lat.device)), use_sr_model=True)
    return dec


def create_super_volume(trainer, images, alpha_range, use_original=False, labels=None, to_cpu=True, *, grid=None):
    """images [z,1,y,x] or [z,y,x] -> {'upsampled_image': [(z-1)(n+1)+1, y, x] (CPU, clamped), 'upsampled_labels': None}.
    ``to_cpu=False`` leaves the result in HBM (callers that go on working on the device; bench.py times it that way).

    ``labels`` [z,1,y,x] or [z,y,x] (class ids; a multi-channel model, reference :23-69): the label maps go in as channel 1 and
    'upsampled_labels' [(z-1)(n+1)+1, y, x] holds the original (``use_original``: float, as given) or reconstructed (int64) label maps
    at the kept slots and, in between, the arg-max maps decoded from the SAME mixed latents as the in-between slices.

    ``grid`` (an ``evaluate.z_grid.ZGrid`` for these z slices; ``alpha_range`` None or empty): the output slices of a target slice
    spacing instead, [grid.J, y, x] -- the input (or reconstructed) slices at the grid's original slots, at every other slot the mix of
    its two neighbours with the slot's own alpha; everything else as above."""
    if grid is not None:
        if alpha_range is not None and len(alpha_range) > 0:
            raise ValueError("alpha_range belongs to the integer grid: with grid=... it must be None or empty (the grid holds the alphas)")
        return _create_super_volume_on_grid(trainer, images, grid, use_original, labels, to_cpu)
    if images.dim() == 3:
        images = torch.unsqueeze(images, dim=1)
    with_labels = labels is not None
    if with_labels and labels.dim() == 3:
        labels = torch.unsqueeze(labels, dim=1)
    dev = trainer.args["device"]
    vol = images.float().to(dev)
    if with_labels:
        if tuple(labels.shape) != tuple(images.shape):
            raise ValueError("labels %s do not match the images %s" % (tuple(labels.shape), tuple(images.shape)))
        vol = torch.cat([vol, labels.float().to(dev)], dim=1)
    Z, _, H, W = vol.shape
    n = len(alpha_range)
    out_labels = None
    with torch.no_grad():
        lat = _encode(trainer, vol)                                   # every slice encoded exactly once
        recon = vol if use_original else trainer.decode(lat, use_sr_model=True)
        if with_labels and not use_original and not isinstance(recon, dict):
            raise ValueError("labels were given, but this model has no label head (MultiChannelAE is the one that has)")
        if not with_labels:
            _no_label_model(recon)
        dec = None
        if Z > 1 and n > 0:
            model = trainer._use_sr_model(True)
            model.eval()
            dec = model.decode_mixes(lat, [float(a) for a in alpha_range]) if hasattr(model, "decode_mixes") else None
            if dec is None:
                zpair = torch.cat([lat[1:], lat[:-1]], dim=0)         # rows i / i+(Z-1): later slice / earlier slice
                mixes = torch.cat([ops.lerp_mix(zpair, float(a), float(1 - a)) for a in alpha_range], dim=0)
                dec = trainer.decode(mixes, use_sr_model=True)        # ONE decoder pass over all (Z-1)*n latents
            if with_labels and not isinstance(dec, dict):
                raise ValueError("labels were given, but this model has no label head (MultiChannelAE is the one that has)")
        if with_labels:
            kept = vol[:, 1] if use_original else recon["pred_labels"][:, 0].float()
            synth = None if dec is None else dec["pred_labels"][:, 0].float()
            out_labels = _interleave(kept, synth, n, (-3.0e38, 3.0e38))          # small integers: exact as floats
            if not use_original:
                out_labels = out_labels.long()
            recon = vol[:, 0:1] if use_original else recon["image"]
            dec = None if dec is None else dec["image"]
        out = _interleave(recon[:, 0], dec, n, (0.0, 1.0))
    if to_cpu:
        out = out.cpu()
        out_labels = None if out_labels is None else out_labels.cpu()
        if vol.is_cuda:
            _hip.check_device_watchdogs("create_super_volume")       # the volume leaves the device here: never a silent garbage volume
    return {"upsampled_image": out, "upsampled_labels": out_labels}


def _create_super_volume_on_grid(trainer, images, grid, use_original, labels, to_cpu):
    """``create_super_volume(..., grid=grid)``: the same steps with the grid's own alphas per gap and assembly by index."""
    if images.dim() == 3:
        images = torch.unsqueeze(images, dim=1)
    with_labels = labels is not None
    if with_labels and labels.dim() == 3:
        labels = torch.unsqueeze(labels, dim=1)
    dev = trainer.args["device"]
    vol = images.float().to(dev)
    if with_labels:
        if tuple(labels.shape) != tuple(images.shape):
            raise ValueError("labels %s do not match the images %s" % (tuple(labels.shape), tuple(images.shape)))
        vol = torch.cat([vol, labels.float().to(dev)], dim=1)
    Z = vol.shape[0]
    if grid.Z != Z:
        raise ValueError("grid is for %d slices, the volume has %d" % (grid.Z, Z))
    out_labels = None
    with torch.no_grad():
        lat = _encode(trainer, vol)                                   # every slice encoded exactly once
        recon = vol if use_original else trainer.decode(lat, use_sr_model=True)
        if with_labels and not use_original and not isinstance(recon, dict):
            raise ValueError("labels were given, but this model has no label head (MultiChannelAE is the one that has)")
        if not with_labels:
            _no_label_model(recon)
        dec = None
        if grid.num_synthesised > 0:
            dec = _decode_on_grid(trainer, lat, grid)
            if not with_labels:
                _no_label_model(dec)
            if with_labels and not isinstance(dec, dict):
                raise ValueError("labels were given, but this model has no label head (MultiChannelAE is the one that has)")
        if with_labels:
            kept = vol[:, 1] if use_original else recon["pred_labels"][:, 0].float()
            synth = None if dec is None else dec["pred_labels"][:, 0]
            out_labels = _assemble(kept, synth, grid, (-3.0e38, 3.0e38))          # small integers: exact as floats
            if not use_original:
                out_labels = out_labels.long()
            recon = vol[:, 0:1] if use_original else recon["image"]
            dec = None if dec is None else dec["image"]
        out = _assemble(recon[:, 0], None if dec is None else dec[:, 0], grid, (0.0, 1.0))
    if to_cpu:
        out = out.cpu()
        out_labels = None if out_labels is None else out_labels.cpu()
        if vol.is_cuda:
            _hip.check_device_watchdogs("create_super_volume")       # the volume leaves the device here: never a silent garbage volume
    return {"upsampled_image": out, "upsampled_labels": out_labels}


# ---- I/O around the path (SimpleITK is optional; .npy volumes work everywhere) -----------------------------------------
def normalize_img(img, perc=(1, 99)):
    lo, hi = np.percentile(img, perc)
    return ((img.astype(img.dtype) - lo) / (hi - lo)).clip(0, 1)


def array_to_torch(np_img):
    np_img = np.asarray(np_img, dtype=np.float32)
    if np_img.max() > 1 or np_img.min() < 0:
        np_img = normalize_img(np_img)
    return torch.from_numpy(np_img).float().unsqueeze(dim=1)


def _sitk():
    try:
        import SimpleITK as sitk
        return sitk
    except ImportError:
        return None


def load_images(input_dir, suffix=".nii*"):
    """[(path, volume)] with volume a SimpleITK image (nii / mha / mhd) or a numpy array (.npy)."""
    input_dir, sitk = Path(input_dir), _sitk()
    files = []
    if sitk is not None:
        for pat in ("*" + suffix, "*.mha", "*.mhd"):
            files = sorted(input_dir.rglob(pat))
            if files:
                return [(f, sitk.ReadImage(str(f))) for f in files]
    else:                                   # no SimpleITK: the built-in NIfTI-1 / MetaImage reader (volume_io.py)
        from . import volume_io
        for pat in ("*" + suffix, "*.mha", "*.mhd"):
            files = sorted(f for f in input_dir.rglob(pat) if not str(f).endswith(".raw"))
            if files:
                return [(f, volume_io.read_volume(f)) for f in files]
    files = sorted(input_dir.rglob("*.npy"))
    if not files:
        raise FileNotFoundError("Error - no files found in {} with extensions nii, mha, mhd or npy".format(input_dir))
    return [(f, np.load(str(f))) for f in files]


def _alpha_range(num_interpolations, grid):
    """The integer grid's alphas, or None where a ``grid`` holds them (``num_interpolations`` must then be None)."""
    if grid is None:
        return np.linspace(0, 1, num_interpolations + 2, endpoint=True)[1:-1]
    if num_interpolations is not None:
        raise ValueError("num_interpolations=%r belongs to the integer grid: with grid=... it must be None" % (num_interpolations,))
    return None


def upsample_volume(trainer, vol_np, num_interpolations, labels_np=None, *, grid=None):
    """[z,y,x] or [t,z,y,x] numpy -> through-plane upsampled numpy with the same leading layout.  ``labels_np`` (same shape, class ids; a
    multi-channel model): returns (volume, label volume as uint8) instead.  ``grid`` (evaluate/z_grid.py, ``num_interpolations`` None): the
    slices of a target spacing; every frame of a 4-D volume gets the same grid."""
    alpha_range = _alpha_range(num_interpolations, grid)
    if labels_np is not None and tuple(labels_np.shape) != tuple(vol_np.shape):
        raise ValueError("the label volume %s does not match the image volume %s" % (tuple(labels_np.shape), tuple(vol_np.shape)))
    if vol_np.ndim == 3:
        if labels_np is None:
            return create_super_volume(trainer, array_to_torch(vol_np), alpha_range, use_original=True, grid=grid)["upsampled_image"].numpy()
        lab = torch.from_numpy(np.ascontiguousarray(labels_np, dtype=np.float32)).unsqueeze(dim=1)
        out = create_super_volume(trainer, array_to_torch(vol_np), alpha_range, use_original=True, labels=lab, grid=grid)
        return out["upsampled_image"].numpy(), np.rint(out["upsampled_labels"].numpy()).astype(np.uint8)
    if labels_np is None:
        return np.stack([upsample_volume(trainer, v, num_interpolations, grid=grid) for v in vol_np])
    pairs = [upsample_volume(trainer, v, num_interpolations, l, grid=grid) for v, l in zip(vol_np, labels_np)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def labels_name(name):
    """vol0.npy -> vol0_labels.npy, p1.nii.gz -> p1_labels.nii.gz"""
    name = str(name)
    for ext in (".nii.gz", ".nii", ".mha", ".mhd", ".npy"):
        if name.endswith(ext):
            return name[:-len(ext)] + "_labels" + ext
    return name + "_labels"


def clean_label_volume(labels_np, largest_component=False, min_component_size=0):
    """A decoded label map can hold small detached islands of a class.  [z,y,x] or [t,z,y,x] class ids -> the same with, per frame and
    class (1 ... the largest label), components of fewer than ``min_component_size`` voxels set to 0 and / or only the largest component
    kept (3-D, face connectivity; evaluate/components.py, on the device).  Shape and dtype are kept; nothing asked for: the input itself."""
    if not largest_component and not min_component_size:
        return labels_np
    from .evaluate.components import keep_largest_component, remove_small_components
    if not labels_np.max() >= 1:
        return labels_np
    classes = list(range(1, int(labels_np.max()) + 1))
    out = []
    for c0 in range(0, len(classes), 8):          # the kernels take eight classes at a time
        chunk, cleaned = classes[c0:c0 + 8], labels_np if not out else out[-1]
        if min_component_size:
            cleaned = remove_small_components(cleaned, int(min_component_size), classes=chunk)
        if largest_component:
            cleaned = keep_largest_component(cleaned, classes=chunk)
        out.append(cleaned)
    return out[-1]


def normalize_on_device(x, perc=(1, 99)):
    """``array_to_torch``'s intensity rule on a device tensor: values outside [0, 1] -> the 1st..99th percentile window mapped to [0, 1]
    and clipped (percentiles with numpy's linear interpolation between the two nearest sorted values)."""
    if not (float(x.max()) > 1 or float(x.min()) < 0):
        return x
    v = x.flatten().sort().values
    n = v.numel()

    def q(p):
        pos = p / 100.0 * (n - 1)
        i = int(np.floor(pos))
        return v[i] + (v[min(i + 1, n - 1)] - v[i]) * float(pos - i)
    lo, hi = q(perc[0]), q(perc[1])
    return ((x - lo) / (hi - lo)).clamp_(0, 1)


def upsample_volume_resampled(trainer, vol_np, num_interpolations, spacing, new_spacing=(1.4, 1.4), clamp_edges=False, *, grid=None):
    """``upsample_volume`` for a volume whose in-plane ``spacing`` (y, x) is not the training spacing: one upload, resample to
    ``new_spacing`` (one launch for all frames and slices), per frame normalise and synthesise (zero-padded to the network's stride where
    the resampled size needs it), resample back to ``spacing`` (one launch), one download.  [z,y,x] or [t,z,y,x] numpy -> numpy with the same leading layout; the in-plane shape is what the round trip of
    ``int(round(n * zoom))`` gives (the input's own for the usual sizes), as in the reference.  ``grid`` as in ``upsample_volume``."""
    from .datasets.common import apply_2d_zoom_3d, apply_2d_zoom_4d
    alpha_range = _alpha_range(num_interpolations, grid)
    zoom = apply_2d_zoom_3d if vol_np.ndim == 3 else apply_2d_zoom_4d
    vol = torch.from_numpy(np.ascontiguousarray(vol_np, dtype=np.float32)).to(trainer.args["device"])
    vol = zoom(vol, spacing, new_spacing, clamp_edges=clamp_edges)
    # the resampled size is whatever the spacing gives (216 x 256 at 1.5625 mm -> 241 x 286): the network halves the image width /
    # latent_width times over, so each frame is zero-padded at the bottom / right to the next multiple of that for the synthesis (after
    # the normalisation, so the percentiles are the image's own) and cropped again before it is resampled back
    m = max(1, int(trainer.args["width"]) // int(trainer.args["latent_width"]))
    H, W = vol.shape[-2:]
    pad = ((-W) % m, (-H) % m)
    frames = [vol] if vol.dim() == 3 else list(vol)
    hr = []
    for f in frames:
        f = normalize_on_device(f)
        if pad != (0, 0):
            f = torch.nn.functional.pad(f, (0, pad[0], 0, pad[1]))
        up = create_super_volume(trainer, f.unsqueeze(1), alpha_range, use_original=True, to_cpu=False, grid=grid)["upsampled_image"]
        hr.append(up[:, :H, :W].contiguous() if pad != (0, 0) else up)
    hr = hr[0] if vol.dim() == 3 else torch.stack(hr)
    out = zoom(hr, new_spacing, spacing, clamp_edges=clamp_edges).cpu().numpy()
    _hip.check_device_watchdogs("upsample_volume_resampled")
    return out


def expand_volume(vol_np, num_interpolations, method, align="itk", radius=5):
    """[z,y,x] or [t,z,y,x] numpy -> the conventional baseline ``method`` along z by ``num_interpolations + 1`` (float32 numpy, same
    leading layout): one upload, one launch for all frames (two for bspline), one download.  Intensities are not normalised or clamped."""
    from .evaluate import z_interp
    if vol_np.ndim not in (3, 4):
        raise ValueError("expected a [z,y,x] or [t,z,y,x] volume, got shape %s" % (vol_np.shape,))
    if not torch.cuda.is_available():
        raise RuntimeError("expand_volume needs the GPU: the HIP path has no CPU fallback")
    x = torch.from_numpy(np.ascontiguousarray(vol_np, dtype=np.float32)).cuda()
    return z_interp.z_expand(x, num_interpolations + 1, method, align=align, radius=radius).cpu().numpy()


def check_method_on_grid(method):
    """The methods that can write the grid of a target slice spacing: the model and the two that ``aesr_reslice_affine`` interpolates."""
    if method not in ("ae", "linear", "nearest"):
        raise ValueError("--method %s cannot be combined with a target slice spacing: aesr_z_expand takes integer factors only "
                         "(ae, linear and nearest can)" % method)


def expand_volume_on_grid(vol_np, grid, method):
    """[z,y,x] or [t,z,y,x] numpy -> the conventional baseline ``method`` (linear or nearest) at the slices of ``grid`` (float32 numpy, same
    leading layout): ``evaluate.reslice`` with the matrix diag(1, 1, target_spacing_z / spacing_z), one upload, one launch for all frames,
    one download.  The grid ends inside the volume, so the zero padding of the linear interpolation is never read."""
    from .evaluate import reslice
    check_method_on_grid(method)
    if method == "ae":
        raise ValueError("expand_volume_on_grid writes a conventional baseline: linear or nearest")
    if vol_np.ndim not in (3, 4):
        raise ValueError("expected a [z,y,x] or [t,z,y,x] volume, got shape %s" % (vol_np.shape,))
    if vol_np.shape[-3] != grid.Z:
        raise ValueError("grid is for %d slices, the volume has %d" % (grid.Z, vol_np.shape[-3]))
    matrix = np.zeros((3, 4), dtype=np.float64)
    matrix[0, 0] = matrix[1, 1] = 1.0
    matrix[2, 2] = grid.target_spacing_z / grid.spacing_z
    return reslice.reslice_affine(np.asarray(vol_np), matrix, (grid.J,) + tuple(vol_np.shape[-2:]), interp=method)


def isotropic_target(spacing_yx, name=""):
    """``--isotropic``: the in-plane spacing the volume is written at is the z spacing asked for; the smaller of the two where the
    pixels are not square (said on stdout)."""
    sy, sx = float(spacing_yx[0]), float(spacing_yx[1])
    if sy != sx:
        print("INFO - {}in-plane spacing {:g} x {:g} mm is not square: --isotropic takes the smaller, {:g} mm".format(
            name and "{}: ".format(name), sy, sx, min(sy, sx)))
    return min(sy, sx)


def parse_args(argv=None):
    """(parser, args) with every check that needs the arguments alone made: ``args.num_interpolations`` is resolved (6 where neither it
    nor a target spacing is given, None with a target) and ``args.on_grid`` says whether a target slice spacing was asked for."""
    p = argparse.ArgumentParser(description="Generate through-plane super-resolved volumes")
    p.add_argument("--method", choices=("ae", "linear", "bspline", "lanczos", "nearest"), default="ae",
                   help="ae: the trained model (default); otherwise a conventional interpolation along z, no --exper_dir needed")
    p.add_argument("--align", choices=("itk", "grid"), default="itk",
                   help="with a conventional --method: itk = SimpleITK's ExpandImageFilter grid (z * (n + 1) slices, half a sample off the "
                        "input slices), grid = input slices at every (n + 1)-th slot ((z - 1) * (n + 1) + 1 slices)")
    p.add_argument("--lanczos_radius", type=int, choices=(3, 4, 5), default=5, help="radius of the Lanczos window for --method lanczos")
    p.add_argument("--resample", action="store_true",
                   help="resample in-plane to --new_spacing before the synthesis and back to the file's own spacing before writing")
    p.add_argument("--new_spacing", type=float, nargs=2, default=[1.4, 1.4], metavar=("Y", "X"),
                   help="in-plane spacing the model was trained at (mm)")
    p.add_argument("--spacing", type=float, nargs=2, default=None, metavar=("Y", "X"),
                   help="in-plane spacing of .npy volumes (they carry none); required for them with --resample")
    p.add_argument("--clamp_edges", action="store_true",
                   help="with --resample: repeat the edge where scipy (and the reference) leave an all-zero last row / column")
    p.add_argument("--exper_dir", type=str, default=None)
    p.add_argument("--model_nbr", type=int, default=None)
    p.add_argument("--num_interpolations", type=int, default=None,
                   help="slices put into every gap (default 6); not together with --target_spacing_z / --isotropic")
    target = p.add_mutually_exclusive_group()
    target.add_argument("--target_spacing_z", type=float, default=None, metavar="MM",
                        help="write slices MM apart instead of an integer number per gap (evaluate/z_grid.py); --method ae, linear or nearest")
    target.add_argument("--isotropic", action="store_true",
                        help="--target_spacing_z = the in-plane spacing the volume is written at (the smaller of y and x)")
    p.add_argument("--spacing_z", type=float, default=None, metavar="MM",
                   help="slice spacing of .npy volumes (they carry none); required for them with --target_spacing_z / --isotropic")
    p.add_argument("--data_input_dir", type=str, default=None)
    p.add_argument("--labels_input_dir", type=str, default=None,
                   help="label volumes (class ids) with the same file names as the images: needs a multi-channel model; writes <name>_labels "
                        "beside every super-resolved image, an integer volume with the image's new z spacing")
    p.add_argument("--largest_component", action="store_true",
                   help="with --labels_input_dir: keep only the largest connected component of every class in <name>_labels")
    p.add_argument("--min_component_size", type=int, default=0, metavar="K",
                   help="with --labels_input_dir: remove components of fewer than K voxels from <name>_labels")
    p.add_argument("--output_dir", type=str, default=None)
    p.add_argument("--save", action="store_true")
    args = p.parse_args(argv)
    if (args.largest_component or args.min_component_size) and args.labels_input_dir is None:
        p.error("--largest_component and --min_component_size clean <name>_labels: they need --labels_input_dir")
    if args.min_component_size < 0:
        p.error("--min_component_size must not be negative")
    if args.method != "ae" and args.resample:
        p.error("--resample belongs to --method ae: a conventional --method interpolates along z only and keeps the in-plane grid")
    if args.method == "ae" and args.exper_dir is None:
        p.error("--method ae needs --exper_dir")
    if args.output_dir is None and args.exper_dir is None:
        p.error("--output_dir is needed when there is no --exper_dir")
    if args.labels_input_dir is not None and (args.method != "ae" or args.resample):
        p.error("--labels_input_dir belongs to --method ae without --resample (label maps are not resampled in-plane)")
    args.on_grid = args.target_spacing_z is not None or args.isotropic
    if args.on_grid and args.num_interpolations is not None:
        p.error("--num_interpolations is the integer grid: it does not go with --target_spacing_z / --isotropic")
    if args.on_grid:
        check_method_on_grid(args.method)
    else:
        args.num_interpolations = 6 if args.num_interpolations is None else args.num_interpolations
    return p, args


def main(argv=None):
    p, args = parse_args(argv)
    on_grid = args.on_grid
    from .kwatsch.get_trainer import get_trainer_dynamic
    tag = "ni0{}".format(args.num_interpolations) if not on_grid else ("iso" if args.isotropic else "sz{:g}".format(args.target_spacing_z))
    out_dir = Path(args.output_dir if args.output_dir is not None else os.path.join(args.exper_dir, tag))
    out_dir.mkdir(parents=True, exist_ok=True)
    images = load_images(Path(args.data_input_dir))
    print("INFO - Found {} files to process in {}".format(len(images), args.data_input_dir))
    if args.resample and args.spacing is None and any(isinstance(img, np.ndarray) for _, img in images):
        p.error("--resample: .npy volumes carry no spacing; give their in-plane spacing with --spacing Y X")
    if on_grid and args.spacing_z is None and any(isinstance(img, np.ndarray) for _, img in images):
        p.error("--target_spacing_z / --isotropic: .npy volumes carry no spacing; give their slice spacing with --spacing_z MM")
    if args.isotropic and args.spacing is None and any(isinstance(img, np.ndarray) for _, img in images):
        p.error("--isotropic: .npy volumes carry no spacing; give their in-plane spacing with --spacing Y X")
    trainer = None
    if args.method == "ae":
        trainer, _ = get_trainer_dynamic(src_path=args.exper_dir, model_nbr=args.model_nbr, model_nbr_sr=None, eval_mode=True)
        multi = hasattr(trainer.model, "decoder_head2")
        if multi and args.labels_input_dir is None:
            p.error("this experiment holds a multi-channel model (image + label map): give the label volumes with --labels_input_dir DIR")
        if not multi and args.labels_input_dir is not None:
            p.error("--labels_input_dir needs a multi-channel model (--dataset ACDCLBL); this experiment's model has no label head")
    label_files = {}
    if args.labels_input_dir is not None:
        label_files = {f.name: lab for f, lab in load_images(Path(args.labels_input_dir))}
        missing = [f.name for f, _ in images if f.name not in label_files]
        if missing:
            p.error("--labels_input_dir holds no label volume named %s" % ", ".join(missing))
    sitk = _sitk()
    results = []
    from . import volume_io

    def label_array(fname):
        lab = label_files[fname.name]
        if isinstance(lab, volume_io.Volume):
            return lab.array
        return lab if isinstance(lab, np.ndarray) else sitk.GetArrayFromImage(lab)

    def file_grid(arr, spacing_yx, spacing_z, fname):
        """One grid per file (every frame of a 4-D file gets it), None for the integer grid; the written in-plane spacing is the file's
        own, also after --resample (the result is resampled back)."""
        if not on_grid:
            return None
        from .evaluate.z_grid import target_grid
        d = isotropic_target(spacing_yx, fname.name) if args.isotropic else args.target_spacing_z
        return target_grid(arr.shape[-3], spacing_z, d)

    def upsample(arr, spacing_yx, fname=None, grid=None):
        if label_files:
            hr_img, hr_lab = upsample_volume(trainer, arr, args.num_interpolations, label_array(fname), grid=grid)
            return hr_img, clean_label_volume(hr_lab, args.largest_component, args.min_component_size)
        if args.method != "ae":
            if grid is not None:
                return expand_volume_on_grid(arr, grid, args.method)
            return expand_volume(arr, args.num_interpolations, args.method, args.align, args.lanczos_radius)
        if not args.resample:
            return upsample_volume(trainer, arr, args.num_interpolations, grid=grid)
        return upsample_volume_resampled(trainer, arr, args.num_interpolations, spacing_yx, args.new_spacing, clamp_edges=args.clamp_edges,
                                         grid=grid)

    for fname, img in images:
        if isinstance(img, volume_io.Volume):
            grid = file_grid(img.array, (img.spacing[1], img.spacing[0]), img.spacing[2], fname)
            hr = upsample(img.array, (img.spacing[1], img.spacing[0]), fname, grid)
            hr, hr_labels = hr if label_files else (hr, None)
            spacing = list(img.spacing)
            spacing[2] = spacing[2] / (args.num_interpolations + 1) if grid is None else grid.target_spacing_z
            results.append((out_dir / fname.name, hr))
            if args.save:
                volume_io.write_volume(out_dir / fname.name, img, hr.astype(np.float32), spacing)
            if hr_labels is not None:
                results.append((out_dir / labels_name(fname.name), hr_labels))
                if args.save:
                    volume_io.write_volume(out_dir / labels_name(fname.name), img, hr_labels, spacing)
        elif isinstance(img, np.ndarray):
            hr = upsample(img, args.spacing, fname, file_grid(img, args.spacing, args.spacing_z, fname))
            hr, hr_labels = hr if label_files else (hr, None)
            results.append((out_dir / fname.name, hr))
            if args.save:
                np.save(str(out_dir / fname.name), hr)
            if hr_labels is not None:
                results.append((out_dir / labels_name(fname.name), hr_labels))
                if args.save:
                    np.save(str(out_dir / labels_name(fname.name)), hr_labels)
        else:
            arr = sitk.GetArrayFromImage(img)
            grid = file_grid(arr, (img.GetSpacing()[1], img.GetSpacing()[0]), img.GetSpacing()[2], fname)
            hr = upsample(arr, (img.GetSpacing()[1], img.GetSpacing()[0]), fname, grid)
            hr, hr_labels = hr if label_files else (hr, None)
            spacing = list(img.GetSpacing())
            zi = 2 if arr.ndim == 3 else 2
            spacing[zi] = spacing[zi] / (args.num_interpolations + 1) if grid is None else grid.target_spacing_z
            if hr.ndim == 4:
                out = sitk.JoinSeries([sitk.GetImageFromArray(v, False) for v in hr])
            else:
                out = sitk.GetImageFromArray(hr)
            out.SetOrigin(img.GetOrigin())
            out.SetDirection(img.GetDirection())
            out.SetSpacing(spacing)
            results.append((out_dir / fname.name, out))
            if args.save:
                sitk.WriteImage(out, str(out_dir / fname.name))
            if hr_labels is not None:
                lab = sitk.JoinSeries([sitk.GetImageFromArray(v, False) for v in hr_labels]) if hr_labels.ndim == 4 else sitk.GetImageFromArray(hr_labels)
                lab.SetOrigin(img.GetOrigin())
                lab.SetDirection(img.GetDirection())
                lab.SetSpacing(spacing)
                results.append((out_dir / labels_name(fname.name), lab))
                if args.save:
                    sitk.WriteImage(lab, str(out_dir / labels_name(fname.name)))
        print("Processed {}".format(fname))
    return results


if __name__ == "__main__":
    main()
