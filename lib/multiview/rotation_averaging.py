"""``lib.multiview.rotation_averaging`` — rotation averaging over a view graph, re-exported from ``structure_from_motion_amd.multiview.rotation_averaging``."""
from structure_from_motion_amd.multiview.rotation_averaging import (GlobalRotations, average_graph_rotations,  # noqa: F401
                                                                    average_rotations, inconsistent_pairs)
