"""The reference's data layer (src/nerfdata) on the device: uint8 images and poses resident, every batch one launch;
PatchLoader: batches of P x P pixel patches over the same dataset; CameraRefiner / IntrinsicsRefiner: learnable poses
and intrinsics behind both loaders;
UnseenViewSampler / UnseenPatchLoader: random poses no photograph was taken from and patches of their rays;
WarpSource: the training views as sources of a depth-warp (reprojection) term."""
from .intrinsics_refine import IntrinsicsRefiner  # noqa: F401
from .pose_refine import CameraRefiner, pose_error  # noqa: F401
from .raydata import FrameLoader, PatchLoader, RayDataset, RayLoader  # noqa: F401
from .unseen import UnseenPatchLoader, UnseenViewSampler  # noqa: F401
from .warp import WarpSource  # noqa: F401
