"""PyTorch adapter of the engine (reference: src/py/ddl/tensorflow/)."""
from ddl.torch.compression import Compression  # noqa: F401
