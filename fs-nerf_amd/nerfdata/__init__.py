"""The reference's data layer (src/nerfdata) on the device: uint8 images and poses resident, every batch one launch;
PatchLoader: batches of P x P pixel patches over the same dataset."""
from .raydata import FrameLoader, PatchLoader, RayDataset, RayLoader  # noqa: F401
