"""``lib.pnp.registration``: absolute pose of every candidate view in one call (structure_from_motion_amd/pnp/registration.py)."""
from structure_from_motion_amd.pnp.registration import (  # noqa: F401
    ViewRegistrations,
    register_views,
)
