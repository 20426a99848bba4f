"""Training of ONE Dense head on frozen features -- a classifier (``LinearProbe``) or an embedding head distilled from a
teacher (``EmbeddingProbe``); the rest of the reference's ``tfimm/train`` is out of scope: DESIGN.md 7."""
from .embedding_probe import DistillResult, EmbeddingProbe  # noqa: F401
from .linear_probe import LinearProbe, StepResult  # noqa: F401
