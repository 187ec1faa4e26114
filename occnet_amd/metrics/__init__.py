"""Evaluation metric of the occupancy-and-flow challenge on the MI355X ray caster."""
from .ray_metrics import (calc_metrics, generate_lidar_rays, main, occ_class_names,  # noqa: F401
                          flow_class_names, process_one_sample)
from .ray_metrics_device import RayMetrics, main_device  # noqa: F401
from .submission_device import SubmissionWriter  # noqa: F401
from .submission_score import SubmissionScore  # noqa: F401
from .voxel_miou import VoxelMIoU  # noqa: F401
