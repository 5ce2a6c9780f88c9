from .rig import Rig, RigCamera  # noqa: F401
