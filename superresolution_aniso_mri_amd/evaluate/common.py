"""Evaluation protocol around the slice synthesis: the reference's ``evaluate/common.py`` on the HIP engine.

``create_super_volume`` (:134-235) is the function the evaluation suites call (``evaluate/create_HR_images.py:309``,
``evaluate/evaluate_image.py:69``): keep every ``downsample_steps``-th slice of a volume, synthesise the slices in between
from the latent mixes, and append the slices that the sub-sampling could not pair.  The synthesis itself is
``generate_hr_volumes.create_super_volume`` (every slice encoded once, all mixes decoded as one batch, interleave and clamp
on the device); this module adds the host-side bookkeeping with the reference's argument names and return keys."""
import os

import numpy as np
import torch

from .. import generate_hr_volumes as _ghv


def save_metrics(output_dir, eval_dataset, metrics_dict, downsample_steps, interpol_method, eval_axis):
    """<output_dir>/results/[<dataset>_]<method>_<k>x[_axis<a>].npz (:11-25); the results directory must not exist twice."""
    output_dir = os.path.join(output_dir, "results")
    if not os.path.isdir(output_dir):
        os.makedirs(output_dir, exist_ok=False)
    name = "{}_{}x.npz".format(interpol_method, downsample_steps) if eval_axis == 0 else \
        "{}_{}x_axis{}.npz".format(interpol_method, downsample_steps, eval_axis)
    if eval_dataset is not None:
        name = "{}_".format(eval_dataset) + name
    path = os.path.join(output_dir, name)
    np.savez(path, **metrics_dict)
    print("INFO - Saved results to {}".format(path))


def strip_conventional_interpolation_results(img3d_sr, img3d_original, expand_factor):
    """Drop the last ``expand_factor`` slices of a conventionally expanded volume and put the last original slice back (:28-32)."""
    return np.concatenate((img3d_sr[:-expand_factor], img3d_original[-1][None]))


def determine_last_slice(orig_num_slices, downsample_steps):
    """Index of the last slice that survives ``[::downsample_steps]`` (:35-38)."""
    return ((int(orig_num_slices) - 1) // int(downsample_steps)) * int(downsample_steps)


def rescale_tensor(p_tensor):
    lo, hi = torch.min(p_tensor), torch.max(p_tensor)
    return torch.clamp((p_tensor - lo) / (hi - lo), min=0, max=1)


def apply_blur_filter(img, sigma=1.):
    """Slice-wise Gaussian blur on the host (:122-126; scipy, used for the blurred conventional baseline only)."""
    from scipy.ndimage import gaussian_filter
    return np.stack([gaussian_filter(img[i], sigma) for i in range(img.shape[0])]) if img.shape[0] else np.zeros_like(img)


def create_recon_from_diff_psize(trainer, test_images, patch_size=(32, 32)):
    """Reconstruct ONE slice [y,x] patch by patch (:52-64): non-overlapping tiles form the batch, the result is the tile
    grid put back together (the part of the slice the tiles cover)."""
    if test_images.dim() > 2:
        test_images = torch.squeeze(test_images)
    return eval_on_different_patch_size(trainer, test_images[None], patch_size)[0]


def eval_on_different_patch_size(trainer, test_images, patch_size=(32, 32)):
    """[z,y,x] CPU tensor -> [z, ny*ph, nx*pw] reconstructions computed on ph x pw tiles (:41-49).  All tiles of all slices
    go through the network as one batch (the reference runs one slice at a time)."""
    if not isinstance(patch_size, tuple):
        patch_size = (int(patch_size), int(patch_size))
    ph, pw = int(patch_size[0]), int(patch_size[1])
    Z, H, W = test_images.shape
    ny, nx = H // ph, W // pw
    dev = trainer.args["device"]
    tiles = test_images.float().to(dev)[:, :ny * ph, :nx * pw].reshape(Z, ny, ph, nx, pw).permute(0, 1, 3, 2, 4)
    rec = trainer.predict(tiles.reshape(Z * ny * nx, 1, ph, pw).contiguous())
    rec = rec.reshape(Z, ny, nx, ph, pw).permute(0, 1, 3, 2, 4).reshape(Z, ny * ph, nx * pw)
    return rec.detach().cpu().contiguous()


def create_super_volume(trainer, images, alpha_range=None, use_original=False, hierarchical=False, downsample_steps=None,
                        generate_inbetween_slices=False, train_patch_size=None, feature_dict=None, labels=None, *, grid=None):
    """images [z,y,x] -> {'upsampled_image' [z',y,x] (CPU, clamped to [0,1]), 'upsampled_labels' None, 'pred_alphas'
    [(z_kept-1)*n, 1, y, x]} with the reference's conventions (:134-235).  ``labels`` [z,y,x] (class ids; a multi-channel model):
    'upsampled_labels' [z',y,x] follows the same slot order -- reconstructed or original label maps at the kept slots, the decoded
    arg-max maps in between, the ORIGINAL label maps of the remainder slices behind them (:220-231):

    * ``generate_inbetween_slices`` without ``downsample_steps`` sub-samples by ``len(alpha_range)+1``;
    * the last ``(z-1) % downsample_steps`` slices cannot be paired: they are cut before sub-sampling and, when in-between
      slices are generated, the ORIGINAL slices are appended after the synthesised stack;
    * ``alpha_range`` defaults to (0.25, 0.5, 0.75); alpha weights the LATER slice of each pair.

    ``grid`` (an ``evaluate.z_grid.ZGrid`` for these z slices): the slices of a target slice spacing instead -- [grid.J, y, x], and
    'pred_alphas' [S, 1, y, x] holds the alpha of each of the S synthesised slices in ascending position.  ``alpha_range`` must then be
    None or empty, and the sub-sampling protocol (``downsample_steps``, ``generate_inbetween_slices``) does not apply: a ValueError."""
    if hierarchical:
        raise NotImplementedError("hierarchical latents are outside this build")
    if images.dim() != 3:
        raise ValueError("create_super_volume expects a [z, y, x] volume, got shape %s" % (tuple(images.shape),))
    if labels is not None and tuple(labels.shape) != tuple(images.shape):
        raise ValueError("labels %s do not match the images %s" % (tuple(labels.shape), tuple(images.shape)))
    if grid is not None:
        if alpha_range is not None and len(alpha_range) > 0:
            raise ValueError("alpha_range belongs to the integer grid: with grid=... it must be None or empty (the grid holds the alphas)")
        if downsample_steps is not None or generate_inbetween_slices:
            raise ValueError("downsample_steps / generate_inbetween_slices sub-sample by an integer: they do not go with grid=...")
        out = _ghv.create_super_volume(trainer, images, None, use_original=use_original, labels=labels, grid=grid)
        alphas = torch.from_numpy(grid.alpha[~grid.is_original].astype(np.float32))
        return {"upsampled_image": out["upsampled_image"], "upsampled_labels": out["upsampled_labels"],
                "pred_alphas": alphas[:, None, None, None].expand(-1, 1, images.shape[1], images.shape[2])}
    if generate_inbetween_slices and downsample_steps is None:
        downsample_steps = int(len(alpha_range) + 1)
    orig, orig_labels, remain = images, labels, 0
    if not generate_inbetween_slices and downsample_steps is not None:
        print("WARNING !!! create_super_volume - downsample steps is not None but generate_inbetween_slices is False!")
    if downsample_steps is not None or generate_inbetween_slices:
        remain = (orig.shape[0] - 1) % downsample_steps
        if remain:
            images = images[:-remain]
            labels = None if labels is None else labels[:-remain]
        images = images[::downsample_steps]
        labels = None if labels is None else labels[::downsample_steps]
    if alpha_range is None:
        alpha_range = [0.25, 0.5, 0.75]
    out = _ghv.create_super_volume(trainer, images, alpha_range, use_original=use_original, labels=labels)
    new_volume, new_labels = out["upsampled_image"], out["upsampled_labels"]
    if generate_inbetween_slices and remain:
        new_volume = torch.clamp(torch.cat([new_volume, orig[-remain:].float().cpu()]), min=0, max=1.)
        if new_labels is not None:
            new_labels = torch.cat([new_labels, orig_labels[-remain:].float().cpu()])       # int64 | float -> float, as in the reference
    pairs = images.shape[0] - 1
    alphas = torch.tensor([float(a) for a in alpha_range], dtype=torch.float32).repeat_interleave(pairs)
    pred_alphas = alphas[:, None, None, None].expand(-1, 1, images.shape[1], images.shape[2])
    return {"upsampled_image": new_volume, "upsampled_labels": new_labels, "pred_alphas": pred_alphas}


def create_simple_interpolation(images, spacing, new_spacing_z=None, expand_factor=None, interpol_filter=None,
                                generate_inbetween_slices=False, *, align="itk", radius=5):
    """The conventional through-plane baselines of the reference (:74-118: SimpleITK's ExpandImageFilter along z) on the device
    (``z_interp.z_expand``, csrc/z_expand.hip).

    :param images: [z, y, x]; a numpy array or CPU tensor (-> numpy ``.array``, through the device) or a CUDA tensor (-> CUDA ``.array``)
    :param spacing: [z, y, x]
    :param new_spacing_z: the z spacing wanted; ``expand_factor = ceil(spacing[0] / new_spacing_z)`` when that is not given
    :param interpol_filter: "nearest", "linear", "bspline" or "lanczos"; None is "lanczos", the reference's default
    :param generate_inbetween_slices: the evaluation protocol (:86-110): keep every ``expand_factor``-th slice, expand those, cut to the
        last kept slice and append the ORIGINAL slices that could not be paired -- the result has as many slices as ``images``
    :param align: "itk" (ExpandImageFilter's grid, half a sample off the input slices) or "grid" (input slices at every f-th slot)
    :param radius: of the Lanczos window, 3, 4 or 5

    Returns a ``z_interp.ExpandedImage`` (``.array``, ``.spacing``, ``.origin``, ``GetSpacing()``, ``GetOrigin()``).  Nothing is clamped:
    the caller clips, as create_HR_images.py:328 does."""
    from . import z_interp
    if new_spacing_z is None and expand_factor is None:
        raise ValueError("create_simple_interpolation needs new_spacing_z or expand_factor")
    method = z_interp.check_method(interpol_filter)
    l_spacing = np.array(spacing, dtype=np.float64)
    if l_spacing.shape != (3,):
        raise ValueError("spacing must be [z, y, x], got %r" % (spacing,))
    expand_factor = int(np.ceil(l_spacing[0] / new_spacing_z)) if expand_factor is None else int(expand_factor)
    z_interp._check(expand_factor, align, radius)
    on_device = torch.is_tensor(images) and images.is_cuda
    if not torch.is_tensor(images):
        images = torch.from_numpy(np.ascontiguousarray(np.asarray(images), dtype=np.float32))
    if images.dim() != 3:
        raise ValueError("create_simple_interpolation expects a [z, y, x] volume, got shape %s" % (tuple(images.shape),))
    if not on_device and not torch.cuda.is_available():
        # a RuntimeError like every "needs the GPU" of the package, of the kind that says what is missing: there is no host implementation
        raise NotImplementedError("create_simple_interpolation needs the GPU: the interpolators are HIP kernels, there is no CPU fallback")
    x = images.detach().to(device=images.device if on_device else "cuda", dtype=torch.float32)
    orig = x
    if generate_inbetween_slices:
        x = x[::expand_factor]
        l_spacing[0] = expand_factor * l_spacing[0]
    new = z_interp.z_expand(x.contiguous(), expand_factor, method, align=align, radius=radius)
    if generate_inbetween_slices:
        last = determine_last_slice(orig.shape[0], expand_factor)
        remain = (orig.shape[0] - 1) % expand_factor
        new = new[:last + 1]
        if remain > 0:
            new = torch.cat([new, orig[-remain:]])
    new_spacing, origin = z_interp.expanded_geometry(l_spacing, expand_factor, align)
    return z_interp.ExpandedImage(new if on_device else new.cpu().numpy(), new_spacing, origin)
