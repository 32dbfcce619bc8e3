"""MI355X-native Neural Scene Flow Fields renderer (one hot path of kwea123/nsff_pl).

Public surface = the reference's own interface for that path:

    from nsff_pl_amd import PosEmbedding, NeRF, render_rays, sample_pdf, interpolate

All arithmetic runs in the gfx950 kernels of ``csrc/`` behind the C-ABI declared in
``include/nsff_render.h``; see DESIGN.md / INTEGRATION.md.
"""
from .config import get_precision, set_precision, get_range_check, set_range_check
from .range_check import RangeFlags, range_flags
from .nerf import NeRF, PosEmbedding
from .rendering import render_rays, sample_pdf
from .interpolation import interpolate
from .frames import (build_records, projection_matrices, resize_images, resize_masks, resize_disps, resize_flows, resize_frames,
                     scaled_intrinsics)
from .sampling import RayBank
from . import flow
from .flow import induced_flow, flow_to_image, flow_epe, epe_from_sums
from . import tracks
from .tracks import advect, draw
from . import motion
from .motion import motion_masks, flow_consistency, fundamental_matrices, propagate
from . import optflow
from .optflow import optical_flow, sequence_flows, refine_flow
from . import depth
from .depth import disparity_maps, triangulate, densify, parallax_matrices, sequence_geometry
from . import panels
from .panels import validation_panels, error_blend
from .lpips import LPIPS
from . import scene
from .scene import nearest_depth, scene_from_colmap, visibility_matrix

__all__ = ["NeRF", "PosEmbedding", "render_rays", "sample_pdf", "interpolate", "set_precision", "get_precision",
           "set_range_check", "get_range_check", "range_flags", "RangeFlags",
           "build_records", "projection_matrices", "RayBank",
           "resize_images", "resize_masks", "resize_disps", "resize_flows", "resize_frames", "scaled_intrinsics",
           "flow", "induced_flow", "flow_to_image", "flow_epe", "epe_from_sums",
           "tracks", "advect", "draw",
           "motion", "motion_masks", "flow_consistency", "fundamental_matrices", "propagate",
           "optflow", "optical_flow", "sequence_flows", "refine_flow",
           "depth", "disparity_maps", "triangulate", "densify", "parallax_matrices", "sequence_geometry",
           "panels", "validation_panels", "error_blend", "LPIPS",
           "scene", "nearest_depth", "scene_from_colmap", "visibility_matrix"]
