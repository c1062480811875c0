"""``lib.bundle.bundle`` — bundle adjustment, re-exported from ``structure_from_motion_amd.bundle.bundle``."""
from structure_from_motion_amd.bundle.bundle import bundle_adjust  # noqa: F401
