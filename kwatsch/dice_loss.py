"""Import-path shim (settings.yaml stores `kwatsch/dice_loss.py`): re-exports superresolution_aniso_mri_amd.kwatsch.dice_loss."""
import importlib as _il

_impl = _il.import_module("superresolution_aniso_mri_amd.kwatsch.dice_loss")
globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
