"""Labelled cardiac volumes (reference module datasets/ACDC/data_with_labels.py: ``ACDCDatasetEDESPairs``): the device-resident loader and
batch assembly live in ``data_device``; this module keeps the reference's module path for them."""
from ...data_device import LabelledTripletAugmenter, load_labelled_volume_dir  # noqa: F401
