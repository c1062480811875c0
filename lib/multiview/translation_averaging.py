"""``lib.multiview.translation_averaging`` — translation averaging over a view graph, re-exported from ``structure_from_motion_amd.multiview.translation_averaging``."""
from structure_from_motion_amd.multiview.translation_averaging import (GlobalPositions, average_graph_translations,  # noqa: F401
                                                                       average_translations, global_poses,
                                                                       inconsistent_pairs)
