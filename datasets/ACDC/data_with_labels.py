"""Import-path shim: re-exports superresolution_aniso_mri_amd.datasets.ACDC.data_with_labels (reference module
datasets/ACDC/data_with_labels.py)."""
import importlib as _il

_impl = _il.import_module("superresolution_aniso_mri_amd.datasets.ACDC.data_with_labels")
globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
