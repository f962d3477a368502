"""Import-path shim (the reference keeps its segmentation scores in `kwatsch/medpy_metrics.py`): re-exports
superresolution_aniso_mri_amd.kwatsch.medpy_metrics."""
import importlib as _il

_impl = _il.import_module("superresolution_aniso_mri_amd.kwatsch.medpy_metrics")
globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
