"""The reference's data layer (src/nerfdata) on the device: uint8 images and poses resident, every batch one launch."""
from .raydata import FrameLoader, RayDataset, RayLoader  # noqa: F401
