"""Training of the classifier head on frozen features (the rest of the reference's ``tfimm/train`` is out of scope:
DESIGN.md 7)."""
from .linear_probe import LinearProbe, StepResult  # noqa: F401
