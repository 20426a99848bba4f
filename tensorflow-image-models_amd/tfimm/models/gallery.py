"""``Gallery``: embeddings to search, resident on the device as bf16, and the fused search over them
(tfimm_hip_embed_search, csrc/embed.hip)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from .model import Tensor

#: what ``Gallery.search`` returns: two ``Tensor`` of shape (B, k) -- int32 gallery rows and their float32 scores --
#: by score descending, equal scores by ascending row
Matches = namedtuple("Matches", ["indices", "scores"])


class Gallery:
    """``Gallery(dim, capacity=0)``: a growing (N, dim) matrix of bf16 rows in device memory with a 16-byte-aligned row
    pitch.  ``add`` appends float32 rows (rounded to nearest even), ``search`` returns for every query the ``k`` rows with
    the largest inner product -- scores and top-k in one pass over the gallery, the (B, N) score matrix never exists.  With
    L2-normalised rows and queries (``EmbeddingModel(..., normalize=True)``) the score is the cosine similarity.  Rows are
    never removed or updated; there is no id / label table: a row's index is its identity."""

    def __init__(self, dim: int, capacity: int = 0):
        from ..engine import ffi
        if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or dim % 16 != 0 \
                or not ffi.EMBED_MIN_E <= dim <= ffi.EMBED_MAX_E:
            raise ValueError(f"Gallery: dim = {dim!r}, must be a multiple of 16 in [{ffi.EMBED_MIN_E}, {ffi.EMBED_MAX_E}] "
                             f"(the domain of tfimm_hip_embed_search)")
        if capacity < 0:
            raise ValueError(f"Gallery: capacity = {capacity}, must not be negative")
        self.dim = int(dim)
        self.pitch = (self.dim + 7) // 8 * 8          # elements: rows start on 16-byte boundaries
        self._capacity = int(capacity)
        self._n = 0
        self._buf = None                              # torch.bfloat16 (capacity, pitch), allocated on the first add
        self._work = {}                               # (B, k) -> workspace of the search (uint8)

    def __len__(self) -> int:
        return self._n

    @property
    def capacity(self) -> int:
        return self._capacity

    def _rows(self, x, what: str):
        """``x`` as a float32 device tensor (n, dim): a ``Tensor`` (or torch tensor) on the GPU stays where it is, host data
        -- an array, a torch tensor on the CPU -- is uploaded"""
        import torch
        if isinstance(x, Tensor):
            t = x.torch()
        elif isinstance(x, torch.Tensor):
            t = x
        else:
            t = np.asarray(x)
        if str(t.dtype).replace("torch.", "") != "float32":
            raise ValueError(f"Gallery.{what}: expected float32, got {t.dtype}")
        if t.ndim != 2 or t.shape[1] != self.dim:
            raise ValueError(f"Gallery.{what}: expected shape (n, {self.dim}), got {tuple(t.shape)}")
        if isinstance(t, np.ndarray) or not t.is_cuda:
            # host data -- an array, or a torch tensor that is not on the GPU -- is uploaded; the kernel never sees a host pointer
            if not torch.cuda.is_available():
                raise RuntimeError("tfimm (MI355X engine) needs a ROCm GPU: no CPU execution path exists.")
            t = (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).to("cuda", non_blocking=True)
        return t

    def add(self, x) -> range:
        """Append the rows of ``x`` -- a ``Tensor`` (it stays on the device) or an array, float32 (n, dim) -- rounded to bf16
        by round-to-nearest-even; returns the ``range`` of their indices."""
        import torch
        t = self._rows(x, "add")
        n = int(t.shape[0])
        if self._n + n >= 2 ** 31:
            raise ValueError("Gallery: at most 2^31 - 1 rows")
        if self._buf is None or self._n + n > self._capacity:
            cap = max(self._n + n, 2 * self._capacity if self._buf is not None else self._capacity, 1)
            buf = torch.zeros((cap, self.pitch), dtype=torch.bfloat16, device=t.device)
            if self._n:
                buf[:self._n].copy_(self._buf[:self._n])
            self._buf, self._capacity = buf, cap
        self._buf[self._n:self._n + n, :self.dim].copy_(t)           # float32 -> bf16: nearest even
        first, self._n = self._n, self._n + n
        return range(first, self._n)

    def numpy(self) -> np.ndarray:
        """the stored rows widened to float32, (len, dim)"""
        if self._buf is None:
            return np.zeros((0, self.dim), np.float32)
        return self._buf[:self._n, :self.dim].float().cpu().numpy()

    def _check_k(self, k) -> None:
        from ..engine import ffi
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"Gallery.search: k must be an integer, got {k!r}")
        if k < 1 or k > self._n or k > ffi.EMBED_MAX_K:
            raise ValueError(f"Gallery.search: k = {k}, must be in [1, min(len = {self._n}, TFIMM_EMBED_MAX_K = {ffi.EMBED_MAX_K})]")

    def search(self, q, k: int = 5, chunk: int = 0) -> Matches:
        """``Matches(indices, scores)`` for float32 queries ``q`` (B, dim), a ``Tensor`` or an array: per query the ``k``
        gallery rows with the largest ``sum_e bf16(q)[e] * row[e]``, score descending, equal scores by ascending row.  Two
        launches on the current stream, behind whatever produced ``q`` there.  ``chunk``: gallery rows per workgroup of the
        first pass, 0 = the library chooses; the result does not depend on it."""
        import torch
        from ..engine import ffi
        self._check_k(k)
        t = self._rows(q, "search").contiguous()
        B, k = int(t.shape[0]), int(k)
        if B > ffi.EMBED_MAX_B:
            raise ValueError(f"Gallery.search: {B} queries, at most TFIMM_EMBED_MAX_B = {ffi.EMBED_MAX_B} per call")
        scores = torch.empty((B, k), dtype=torch.float32, device=t.device)
        indices = torch.empty((B, k), dtype=torch.int32, device=t.device)
        if B == 0:
            return Matches(Tensor(indices), Tensor(scores))
        need = ffi.lib.tfimm_hip_embed_search_workspace(B, self._n, self.dim, k, chunk)
        if need < 0:
            ffi.check(int(need), "tfimm_hip_embed_search_workspace")
        work = self._work.get((B, k))
        if work is None or work.numel() < need:
            work = self._work[(B, k)] = torch.empty(int(need), dtype=torch.uint8, device=t.device)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_embed_search(t.data_ptr(), self.dim, B, self._buf.data_ptr(), self.pitch, self._n, self.dim, k,
                                                 int(chunk), scores.data_ptr(), indices.data_ptr(), work.data_ptr(),
                                                 work.numel(), st), "tfimm_hip_embed_search")
        return Matches(Tensor(indices), Tensor(scores))
