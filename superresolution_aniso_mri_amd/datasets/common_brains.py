"""Brain volumes: thick-slice simulation on the device and the small host helpers around it -- the reference's
``datasets/common_brains.py:19-44,117-144``.

The reference does not train brain models on scanner data as it arrives: ``simulate_thick_slices`` blurs every (y, x) column along z
with ``scipy.ndimage.gaussian_filter1d(column, sigma = slice_thickness / 2.355)`` (the slice profile as a Gaussian whose FWHM is the
thickness), the result is saved as ``*_3mm.nii.gz``, loaded with ``[::downsample_steps]`` and rescaled by its (0, 100) percentiles.
Here the blur is ONE launch of ``aesr_thick_slices`` (csrc/thick_slices.hip, include/aesr_hip_dataprep.h); with ``z_step = k`` it computes
only the slices ``[::k]`` keeps.  The weights are scipy's, made on the host in float64 (``datasets.common.gaussian_weights``); the kernel
accumulates in double in scipy's order and rounds once.  There is no CPU fallback: a numpy array goes to the device and comes back."""
import numpy as np
import torch

from .. import _hip
from .._hip import check, lib, ptr, stream
from .common import gaussian_weights

MAX_RADIUS = 16         # TS_MAXR of csrc/thick_slices.hip: slice_thickness <= 9.7
FWHM = 2.355            # FWHM = 2.355 sigma
BRAIN_DATASETS = ("OASIS", "dHCP", "ADNI")


def get_file_suffix_blurred(dataset_name, file_suffix, downsample_steps):
    """File suffix of the blurred copy of a volume (datasets/common_brains.py:19-34)."""
    if dataset_name == "OASIS":
        return file_suffix.replace(".nii.gz", "") + "_{}mm.nii.gz".format(downsample_steps)
    if dataset_name == "dHCP":
        # slices are 0.5 mm thick: the thickness in mm is half the number of steps
        return file_suffix.replace(".nii.gz", "") + "_{:.1f}mm.nii.gz".format(downsample_steps / 2)
    if dataset_name == "MNIST3D":
        return file_suffix
    if dataset_name == "ADNI":
        return "_{}mm.nii".format(downsample_steps)
    raise NotImplementedError("Error - get_file_suffix_blurred - {} dataset not supported!".format(dataset_name))


def default_slice_thickness(dataset_name, downsample_steps):
    """The thickness the reference's dataset creators blur with: ``downsample_steps`` (OASIS/dataset.py:114, ADNI) and
    ``downsample_steps / 2`` for dHCP (dHCP/dataset.py:27: 0.5 mm voxels)."""
    return downsample_steps / 2 if dataset_name == "dHCP" else downsample_steps


def determine_interpol_coefficients(sliceid_from, sliceid_to, sliceid_between):
    """(alpha_from, alpha_to) from the slice distances (datasets/common_brains.py:117-119), in the reference's arithmetic."""
    gap = sliceid_to - sliceid_from
    return 1 - ((sliceid_between - sliceid_from) * 1/gap), 1 - ((sliceid_to - sliceid_between) * 1/gap)


def thick_slices(x, slice_thickness, z_step=1):
    """x: CUDA float32 [Z, H, W], contiguous -> new CUDA tensor [ceil(Z / z_step), H, W] = blur(x)[::z_step].  One launch, no
    synchronisation; x is not modified."""
    _hip.require_gpu_tensor(x, "x")
    if x.dim() != 3:
        raise ValueError("expected [Z, H, W], got %s" % (tuple(x.shape),))
    if not float(slice_thickness) > 0:
        raise ValueError("slice_thickness=%r must be positive" % (slice_thickness,))
    Z, H, W = (int(s) for s in x.shape)
    z_step = int(z_step)
    w, r = gaussian_weights(float(slice_thickness) / FWHM)
    Zo = int(lib.aesr_thick_slices_out_slices(Z, z_step))
    if Zo < 1 or H < 1 or W < 1:
        raise ValueError("nothing to blur: shape %s, z_step %d" % (tuple(x.shape), z_step))
    out = torch.empty((Zo, H, W), device=x.device, dtype=torch.float32)
    w = np.ascontiguousarray(w, np.float64)
    with torch.cuda.device(x.device):
        check(lib.aesr_thick_slices(ptr(x), ptr(out), Z, H, W, z_step, w.ctypes.data_as(_hip.DP), r, stream()), "aesr_thick_slices")
    return out


def simulate_thick_slices(img3d, slice_thickness, z_step=1):
    """The reference's ``simulate_thick_slices`` (datasets/common_brains.py:37-44) on the device.

    :param img3d: [z, y, x]; a numpy array (-> float32 numpy array) or a CUDA tensor (-> CUDA tensor, no host round trip)
    :param slice_thickness: FWHM of the Gaussian slice profile in voxels along z (sigma = slice_thickness / 2.355)
    :param z_step: 1 gives the whole blurred volume; k gives ``blurred[::k]`` at 1/k of the work

    The device path takes float32: anything else is cast to float32 first.  The input is left untouched."""
    on_device = torch.is_tensor(img3d)
    if on_device:
        if not img3d.is_cuda:
            raise RuntimeError("a tensor must live on the GPU (got %s); pass a numpy array for host data" % img3d.device)
        x = img3d
    else:
        img3d = np.asarray(img3d)
        if img3d.ndim != 3:
            raise ValueError("expected a 3-D array [z, y, x], got shape %s" % (tuple(img3d.shape),))
        if not torch.cuda.is_available():
            raise RuntimeError("simulate_thick_slices needs the GPU: the HIP path has no CPU fallback")
        x = torch.from_numpy(np.ascontiguousarray(img3d, dtype=np.float32)).cuda()
    if x.dim() != 3:
        raise ValueError("expected a 3-D array [z, y, x], got shape %s" % (tuple(x.shape),))
    out = thick_slices(x.to(torch.float32).contiguous(), slice_thickness, z_step)
    return out if on_device else out.cpu().numpy()


def rescale_intensities(img, percs=(0, 100)):
    """datasets/common.py rescale_intensities of the reference with the brain loaders' default window (the whole range)."""
    from ..data_device import rescale_intensities as _rescale
    return _rescale(img, percs)


def process_img(np_image, transform, do_downsample, downsample_steps, rescale_int, int_perc=(0, 100)):
    """datasets/common_brains.py:136-144: transform, then ``[::downsample_steps]``, then ``rescale_intensities``."""
    if transform is not None:
        np_image = transform({"image": np_image})["image"]
    if do_downsample:
        np_image = np_image[::int(downsample_steps)]
    if rescale_int:
        np_image = rescale_intensities(np_image, percs=int_perc)
    return np_image


def minmax_rescale_(x):
    """``rescale_intensities(percs=(0, 100))`` of a device tensor, in place: (x - min) / (max - min), clipped to [0, 1].  The 0th and
    100th percentiles are the minimum and the maximum, so no sort is needed.  fp32 throughout (the reference's numpy arithmetic promotes to
    float64 there; the device result is within 1.2e-7 of it: three fp32 roundings of values <= 1)."""
    lo, hi = torch.aminmax(x)
    return x.sub_(lo).div_(hi - lo).clamp_(0, 1)


def lr_volume_on_device(arr, slice_thickness, downsample_steps, rescale=True, device="cuda"):
    """One upload, one ``aesr_thick_slices(z_step = downsample_steps)`` and one min / max rescale on the device: the [Zo, H, W] float32
    CUDA tensor the reference would have loaded from its blurred file (``process_img`` with ``do_downsample`` and ``rescale_int``).
    ``slice_thickness`` None: the volume is blurred already, only ``[::downsample_steps]`` and the rescale are applied."""
    x = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(device)
    if slice_thickness is None:
        x = x[::int(downsample_steps)].contiguous()
    else:
        x = thick_slices(x, slice_thickness, int(downsample_steps))
    return minmax_rescale_(x) if rescale else x
