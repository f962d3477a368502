"""Import-path shim: re-exports superresolution_aniso_mri_amd.datasets.common_brains (reference module datasets/common_brains.py)."""
import importlib as _il

_impl = _il.import_module("superresolution_aniso_mri_amd.datasets.common_brains")
globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
