from .rig import Rig, RigCalibrationResult, RigCamera  # noqa: F401
