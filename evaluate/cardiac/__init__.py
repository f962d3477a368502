"""Import-path shim: the reference's evaluate.cardiac package, served by superresolution_aniso_mri_amd.evaluate.cardiac."""
