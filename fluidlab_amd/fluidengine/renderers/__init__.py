from .hip_renderer import HIPRenderer  # noqa: F401
