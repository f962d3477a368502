"""Import-path shim: re-exports superresolution_aniso_mri_amd.evaluate.cardiac.resample_sax_to_lax (reference module
evaluate/cardiac/resample_sax_to_lax.py)."""
import importlib as _il

_impl = _il.import_module("superresolution_aniso_mri_amd.evaluate.cardiac.resample_sax_to_lax")
globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
