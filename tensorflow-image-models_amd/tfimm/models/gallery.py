"""``Gallery``: embeddings to search, resident on the device as bf16, and the fused search over them
(tfimm_hip_embed_search, csrc/embed.hip; for up to 256 neighbours tfimm_hip_embed_search_wide,
csrc/embed_wide.hip; coarse to fine over an fp8 copy of the rows tfimm_hip_embed_search_coarse,
csrc/embed_coarse.hip); with a label per row, the matches turned into classes and
scored on the device (tfimm_hip_knn_vote / tfimm_hip_knn_score, csrc/knn.hip); and the rows grouped on the
device -- every row to its best centroid, the mean of every group -- into class prototypes and spherical k-means
(tfimm_hip_cluster_assign / tfimm_hip_segment_mean, csrc/cluster.hip).  ``build_index`` turns the groups into
the inverted lists of a ``GalleryIndex`` (gallery_index.py), the one search that does not read every row."""
import ctypes as C
from collections import namedtuple

import numpy as np

from .model import Tensor

#: what ``Gallery.search`` returns: two ``Tensor`` of shape (B, k) -- int32 gallery rows and their float32 scores --
#: by score descending, equal scores by ascending row
Matches = namedtuple("Matches", ["indices", "scores"])

#: what ``Gallery.vote`` / ``Gallery.classify`` return: ``Tensor`` on the device -- int32 classes, float32 values and int32
#: counts, each (B, top), by value descending, equal values by ascending class, empty slots (-1, 0, 0); float32 total (B,)
Votes = namedtuple("Votes", ["classes", "values", "counts", "total"])

#: what ``Gallery.assign`` returns: two ``Tensor`` (len,) on the device -- the int32 row of the best centroid of every gallery
#: row (of equal scores the lowest) and its float32 score
Assigned = namedtuple("Assigned", ["clusters", "scores"])

#: what ``Gallery.kmeans`` returns: ``centroids`` a labelled ``Gallery`` (label j on row j); ``assignment`` int32 (len,),
#: ``scores`` float32 (len,), ``counts`` int32 (n_clusters,) of the rows against those centroids; ``moved`` int32 (iters,)
Clusters = namedtuple("Clusters", ["centroids", "assignment", "scores", "counts", "moved"])

_REDUCE = ("sum", "max")          # TFIMM_KNN_SUM, TFIMM_KNN_MAX
_METHODS = ("auto", "list", "buffer")

#: the smallest ``k <= 64`` from which ``Gallery.search`` (``search_with(method="auto")``) takes the buffer path
#: (tfimm_hip_embed_search_wide): the smallest probed k from which its median lay below the list path's minimum at every shape of that k in
#: profiles/search_wide_probe.txt (k = 5 loses, k = 20 and k = 64 win); 65 would keep the list path throughout
SEARCH_BUFFER_FROM_K = 20


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _row_labels(labels, n, what):
    """``labels`` of ``n`` gallery rows in the forms ``meter._labels`` takes.  Host labels are validated -- -1: the row never
    votes; below -1 or above 2^31 - 1: ``ValueError`` --, device labels are not looked at (no synchronisation).  Returns the
    callable that does the device part."""
    import torch
    from .meter import _labels
    upload = _labels(labels, n, what)
    y = labels.torch() if isinstance(labels, Tensor) else labels
    if not (isinstance(y, torch.Tensor) and y.is_cuda):
        a = y.numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        if a.size and (int(a.min()) < -1 or int(a.max()) > 2 ** 31 - 1):
            raise ValueError(f"{what}: labels: a gallery label is a class in [0, 2^31 - 1] or -1 (the row never votes), got "
                             f"values in [{int(a.min())}, {int(a.max())}]")
    return upload


def _merge_launch(sets, k: int):
    """tfimm_hip_matches_merge on the current stream: ``sets`` is 1 to 8 triples (int32 indices (B, k_s), float32 scores
    (B, k_s), base), contiguous torch tensors on one device, B >= 1 -> (indices, scores) torch tensors (B, k); no
    synchronisation"""
    import torch
    from ..engine import ffi
    B, dev = int(sets[0][0].shape[0]), sets[0][0].device
    indices = torch.empty((B, k), dtype=torch.int32, device=dev)
    scores = torch.empty((B, k), dtype=torch.float32, device=dev)
    arr = (ffi.MatchSet * len(sets))()
    for rec, (i, s, base) in zip(arr, sets):
        rec.scores, rec.indices, rec.ld, rec.k, rec.base = s.data_ptr(), i.data_ptr(), int(i.shape[1]), int(i.shape[1]), int(base)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ffi.check(ffi.lib.tfimm_hip_matches_merge(arr, len(sets), B, int(k), scores.data_ptr(), indices.data_ptr(), int(k), st),
              "tfimm_hip_matches_merge")
    return indices, scores


def merge_matches(parts, bases=None, k=None) -> Matches:
    """The ``k`` best of several ``Matches`` per query, joined on the device (tfimm_hip_matches_merge, csrc/embed_merge.hip;
    DESIGN.md 3.30): ``parts`` is a sequence of 1 to 8 ``Matches`` on one device with the same number of queries -- the
    results of the shards of a gallery, of several galleries, of a second device after a copy --, ``bases`` the row offset of
    each part in the common numbering (integers >= 0; default all 0), ``k`` the width of the result (default: the widest part;
    ``1 <= k <= 256``).  Entries with index -1 are no candidates; the result is ordered as ``Gallery.search`` orders --
    score descending, equal scores by ascending row (after the base) --, scores keep their bits, and the slots behind the last
    candidate hold -1 / -inf.  The parts must be what the searches return -- valid entries first, in that order -- and the
    rows of a query distinct across the parts; otherwise the result is unspecified.  One launch on the current stream,
    nothing goes to the host; every ``ValueError`` comes before any device work."""
    import torch
    from ..engine import ffi
    what = "merge_matches"
    if isinstance(parts, Matches) or not isinstance(parts, (list, tuple)):
        raise ValueError(f"{what}: parts must be a sequence of Matches, got {type(parts).__name__}")
    if not 1 <= len(parts) <= ffi.MERGE_MAX_SETS:
        raise ValueError(f"{what}: parts: {len(parts)} Matches, must be 1 to TFIMM_MERGE_MAX_SETS = {ffi.MERGE_MAX_SETS}")
    if bases is None:
        bases = [0] * len(parts)
    try:
        bases = list(bases)
    except TypeError:
        raise ValueError(f"{what}: bases must be a sequence of integers, got {bases!r}") from None
    if len(bases) != len(parts):
        raise ValueError(f"{what}: bases: {len(bases)} offsets for {len(parts)} parts")
    for n, base in enumerate(bases):
        if not _is_int(base) or base < 0 or base >= 2 ** 31:
            raise ValueError(f"{what}: bases[{n}] = {base!r}, must be an integer in [0, 2^31)")
    sets = []
    for n, m in enumerate(parts):
        try:
            i, s = (x.torch() if isinstance(x, Tensor) else x for x in m)
            ok = isinstance(i, torch.Tensor) and isinstance(s, torch.Tensor)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{what}: parts[{n}] must be the Matches(indices, scores) of a search, got {type(m).__name__}")
        if i.dtype != torch.int32 or s.dtype != torch.float32 or i.ndim != 2 or i.shape != s.shape:
            raise ValueError(f"{what}: parts[{n}]: expected int32 indices and float32 scores of one shape (B, k), got {i.dtype} "
                             f"{tuple(i.shape)} and {s.dtype} {tuple(s.shape)}")
        if not 1 <= i.shape[1] <= ffi.EMBED_WIDE_MAX_K:
            raise ValueError(f"{what}: parts[{n}] with k = {i.shape[1]}, must be in [1, TFIMM_EMBED_WIDE_MAX_K = {ffi.EMBED_WIDE_MAX_K}]")
        sets.append((i, s, int(bases[n])))
    B = int(sets[0][0].shape[0])
    for n, (i, _, _) in enumerate(sets):
        if int(i.shape[0]) != B:
            raise ValueError(f"{what}: parts[{n}] holds {int(i.shape[0])} queries, parts[0] holds B = {B}")
    if B > ffi.EMBED_MAX_B:
        raise ValueError(f"{what}: {B} queries, at most TFIMM_EMBED_MAX_B = {ffi.EMBED_MAX_B} per call")
    if k is None:
        k = max(int(i.shape[1]) for i, _, _ in sets)
    if not _is_int(k):
        raise ValueError(f"{what}: k must be an integer, got {k!r}")
    if k < 1 or k > ffi.EMBED_WIDE_MAX_K:
        raise ValueError(f"{what}: k = {k}, must be in [1, TFIMM_EMBED_WIDE_MAX_K = {ffi.EMBED_WIDE_MAX_K}]")
    dev = sets[0][0].device
    for n, (i, s, _) in enumerate(sets):
        if not (i.is_cuda and s.is_cuda) or i.device != dev or s.device != dev:
            raise ValueError(f"{what}: parts[{n}] must be on the device, and all parts on one (what Gallery.search returns)")
    k = int(k)
    if B == 0:
        return Matches(Tensor(torch.empty((0, k), dtype=torch.int32, device=dev)), Tensor(torch.empty((0, k), dtype=torch.float32, device=dev)))
    with torch.cuda.device(dev):
        indices, scores = _merge_launch([(i.contiguous(), s.contiguous(), b) for i, s, b in sets], k)
    return Matches(Tensor(indices), Tensor(scores))


class Gallery:
    """``Gallery(dim, capacity=0)``: a growing (N, dim) matrix of bf16 rows in device memory with a 16-byte-aligned row
    pitch.  ``add`` appends float32 rows (rounded to nearest even), ``search`` returns for every query the ``k`` rows with
    the largest inner product -- scores and top-k in one pass over the gallery, the (B, N) score matrix never exists.  With
    L2-normalised rows and queries (``EmbeddingModel(..., normalize=True)``) the score is the cosine similarity.  Rows are
    never removed or updated.

    Without labels a row's index is its identity.  ``add(x, labels)`` on an empty gallery makes it a LABELLED one: an int32
    label per row lives next to the rows on the device (several rows per person, hundreds per class), every later ``add``
    needs labels, and one more launch behind the search turns the matches into classes: ``vote`` / ``classify`` -- a weighted
    vote, or the best row per identity -- and ``evaluate``, which scores a labelled batch of queries into a ``tfimm.Meter``:
    the kNN probe of an embedding, with no host trip per batch.

    Nobody has to organise the gallery beforehand: ``prototypes`` turns a labelled gallery into one row per class (search
    ``nb_classes`` rows at ``k = 1`` instead of every row at ``k = 20``), ``kmeans`` groups an unlabelled one into
    pseudo-identities, ``assign`` gives every row its best centroid, and ``set_labels`` hands the groups to the kNN end."""

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
        self._work = {}                               # (B, k, path) -> workspace of the search (uint8)
        self._labelled = False
        self._lab = None                              # torch.int32 (capacity,), a labelled gallery's label per row
        self._coarse = False                          # build_coarse: an fp8 copy of the rows for search_coarse
        self._codes = None                            # torch.uint8 (capacity, dim): e4m3fn codes, row pitch dim (a multiple of 16)
        self._exps = None                             # torch.int8 (capacity,): the power of two of every row's scale
        self._work_coarse = {}                        # (B, k, candidates) -> workspace of search_coarse (uint8)

    def __len__(self) -> int:
        return self._n

    @property
    def capacity(self) -> int:
        return self._capacity

    @property
    def labelled(self) -> bool:
        """whether the rows carry labels (``add(x, labels)`` on the empty gallery)"""
        return self._labelled

    def _rows(self, x, what: str):
        """``x`` as a float32 device tensor (n, dim): a ``Tensor`` (or torch tensor) on the GPU stays where it is, host data
        -- an array, a torch tensor on the CPU -- is uploaded"""
        return self._upload_rows(self._check_rows(x, what))

    def _check_rows(self, x, what: str):
        """the ``ValueError`` part of ``_rows``: ``x`` as the (n, dim) float32 array or torch tensor it is, not moved"""
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
        return t

    @staticmethod
    def _upload_rows(t):
        import torch
        if isinstance(t, np.ndarray) or not t.is_cuda:
            # host data -- an array, or a torch tensor that is not on the GPU -- is uploaded; the kernel never sees a host pointer
            if not torch.cuda.is_available():
                raise RuntimeError("tfimm (MI355X engine) needs a ROCm GPU: no CPU execution path exists.")
            t = (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).to("cuda", non_blocking=True)
        return t

    def add(self, x, labels=None) -> range:
        """Append the rows of ``x`` -- a ``Tensor`` (it stays on the device) or an array, float32 (n, dim) -- rounded to bf16
        by round-to-nearest-even; returns the ``range`` of their indices.  ``labels``: one class per row -- a list, an integer
        array or a torch int32 / int64 tensor on either side, (n,).  The first ``add`` with labels, on an empty gallery,
        makes the gallery a labelled one; from then on every ``add`` needs them, and an unlabelled gallery that holds rows
        takes none.  -1 marks a row that is searched but never votes; host labels below -1 or above 2^31 - 1 are refused,
        device labels are not looked at (no synchronisation; a negative one never votes)."""
        t = self._check_rows(x, "add")
        n = int(t.shape[0])
        if self._n + n >= 2 ** 31:
            raise ValueError("Gallery: at most 2^31 - 1 rows")
        up_labels = None
        if labels is None:
            if self._labelled:
                raise ValueError(f"Gallery.add: this gallery is labelled: {n} rows need {n} labels")
        else:
            if not self._labelled and self._n:
                raise ValueError(f"Gallery.add: labels for a gallery that holds {self._n} rows without: a gallery is labelled "
                                 f"from its first row on, or not at all")
            up_labels = _row_labels(labels, n, "Gallery.add")
        return self._store(t, up_labels, n)

    def _store(self, t, up_labels, n: int) -> range:
        """the device part of ``add``"""
        import torch
        t = self._upload_rows(t)
        if self._buf is None or self._n + n > self._capacity:
            cap = max(self._n + n, 2 * self._capacity if self._buf is not None else self._capacity, 1)
            buf = torch.zeros((cap, self.pitch), dtype=torch.bfloat16, device=t.device)
            if self._n:
                buf[:self._n].copy_(self._buf[:self._n])
            self._buf, self._capacity = buf, cap
        self._buf[self._n:self._n + n, :self.dim].copy_(t)           # float32 -> bf16: nearest even
        if self._coarse:                                             # the fp8 copy grows with the rows and takes the new ones
            self._grow_coarse()
            self._quantize(self._n, n)
        if up_labels is not None:
            self._labelled = True
            if self._lab is None or self._lab.shape[0] < self._capacity:     # grows with the rows
                lab = torch.full((self._capacity,), -1, dtype=torch.int32, device=t.device)
                if self._n:
                    lab[:self._n].copy_(self._lab[:self._n])
                self._lab = lab
            self._lab[self._n:self._n + n].copy_(up_labels())
        first, self._n = self._n, self._n + n
        return range(first, self._n)

    def labels(self) -> np.ndarray:
        """the labels of the rows, numpy int32 (len,) (one device -> host copy)"""
        self._need_labels("Gallery.labels")
        if self._lab is None:
            return np.zeros(0, np.int32)
        return self._lab[:self._n].cpu().numpy()

    def labels_of(self, indices) -> Tensor:
        """the labels of the rows ``indices`` -- a ``Tensor`` (``Matches.indices``), a torch tensor or an integer array of any
        shape -- as an int32 ``Tensor`` of that shape on the device: a torch gather, no kernel of ours.  The entries are not
        looked at on the host; one outside [0, len) gives -1."""
        import torch
        self._need_labels("Gallery.labels_of")
        i = indices.torch() if isinstance(indices, Tensor) else indices
        if not isinstance(i, torch.Tensor):
            i = torch.from_numpy(np.ascontiguousarray(np.asarray(i)))
        if i.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"Gallery.labels_of: indices: expected int32 or int64, got {i.dtype}")
        if not self._n:
            raise ValueError("Gallery.labels_of: the gallery is empty")
        i = i.to(self._lab.device).long()
        inside = (i >= 0) & (i < self._n)
        return Tensor(torch.where(inside, self._lab[i.clamp(0, self._n - 1)], torch.full_like(i, -1, dtype=torch.int32)))

    def _need_labels(self, what: str) -> None:
        if not self._labelled:
            raise ValueError(f"{what}: this gallery has no labels (add(x, labels) on the empty gallery makes it a labelled one)")

    def numpy(self) -> np.ndarray:
        """the stored rows widened to float32, (len, dim)"""
        if self._buf is None:
            return np.zeros((0, self.dim), np.float32)
        return self._buf[:self._n, :self.dim].float().cpu().numpy()

    def _route(self, k, method="auto") -> str:
        """every ``ValueError`` of ``search`` about ``k`` and ``method``; returns the path the search takes: ``"list"``
        (tfimm_hip_embed_search) or ``"buffer"`` (tfimm_hip_embed_search_wide).  No device work."""
        from ..engine import ffi
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"Gallery.search: k must be an integer, got {k!r}")
        if method not in _METHODS:
            raise ValueError(f"Gallery.search: method = {method!r}, must be one of {', '.join(map(repr, _METHODS))}")
        if k < 1 or k > self._n or k > ffi.EMBED_WIDE_MAX_K:
            raise ValueError(f"Gallery.search: k = {k}, must be in [1, min(len = {self._n}, TFIMM_EMBED_WIDE_MAX_K = "
                             f"{ffi.EMBED_WIDE_MAX_K})]")
        if method == "list":
            if k > ffi.EMBED_MAX_K:
                raise ValueError(f"Gallery.search: k = {k} with method='list', whose limit is TFIMM_EMBED_MAX_K = {ffi.EMBED_MAX_K} "
                                 f"(method='buffer' or 'auto' go up to {ffi.EMBED_WIDE_MAX_K})")
            return "list"
        wide = int(ffi.lib.tfimm_hip_embed_search_wide_max_k(self.dim))     # what the LDS next to a query tile of this width holds
        if method == "buffer" and k > wide:
            raise ValueError(f"Gallery.search: k = {k} with method='buffer': rows of dim {self.dim} allow "
                             f"{'k <= ' + str(wide) if wide > 0 else 'no k'} on this path (tfimm_hip_embed_search_wide_max_k)")
        if k > ffi.EMBED_MAX_K and k > wide:
            raise ValueError(f"Gallery.search: k = {k}: rows of dim {self.dim} allow k <= {max(wide, ffi.EMBED_MAX_K)} "
                             f"(tfimm_hip_embed_search_wide_max_k({self.dim}) = {wide}, TFIMM_EMBED_MAX_K = {ffi.EMBED_MAX_K})")
        if method == "buffer" or k > ffi.EMBED_MAX_K or (SEARCH_BUFFER_FROM_K <= k <= wide):
            return "buffer"
        return "list"

    def search(self, q, k: int = 5, chunk: int = 0) -> Matches:
        """``Matches(indices, scores)`` for float32 queries ``q`` (B, dim), a ``Tensor`` or an array: per query the ``k``
        gallery rows with the largest ``sum_e bf16(q)[e] * row[e]``, score descending, equal scores by ascending row.  Two
        launches on the current stream, behind whatever produced ``q`` there.  ``chunk``: gallery rows per workgroup of the
        first pass, 0 = the library chooses; the result does not depend on it.

        ``k`` goes up to 256 (``TFIMM_EMBED_WIDE_MAX_K``; at ``dim > 768`` up to what
        ``tfimm_hip_embed_search_wide_max_k(dim)`` allows, and never less than 64).  This is ``search_with(q, k, chunk,
        method="auto")``: the route changes time only.  ``vote`` takes ``Matches`` of at most 64 columns: ``vote``,
        ``classify`` and ``evaluate`` keep ``k <= 64``."""
        return self.search_with(q, k, chunk, "auto")

    def search_with(self, q, k: int = 5, chunk: int = 0, method: str = "auto") -> Matches:
        """``search`` by a chosen selection.  ``method``: ``"list"`` keeps the ``k`` best in sorted lists
        (tfimm_hip_embed_search, ``k <= 64``), ``"buffer"`` in unsorted buffers that are pruned (tfimm_hip_embed_search_wide,
        ``k <= 256``); both give the same bits, so ``"auto"`` -- the buffer path for ``k > 64`` and from
        ``SEARCH_BUFFER_FROM_K`` upwards, the list path below and wherever the width allows no buffers -- changes time only.
        ``search`` keeps the signature it had; the choice lives here."""
        import torch
        from ..engine import ffi
        path = self._route(k, method)
        t = self._rows(q, "search").contiguous()
        B, k = int(t.shape[0]), int(k)
        if B > ffi.EMBED_MAX_B:
            raise ValueError(f"Gallery.search: {B} queries, at most TFIMM_EMBED_MAX_B = {ffi.EMBED_MAX_B} per call")
        scores = torch.empty((B, k), dtype=torch.float32, device=t.device)
        indices = torch.empty((B, k), dtype=torch.int32, device=t.device)
        if B == 0:
            return Matches(Tensor(indices), Tensor(scores))
        name = "tfimm_hip_embed_search" if path == "list" else "tfimm_hip_embed_search_wide"
        need = getattr(ffi.lib, name + "_workspace")(B, self._n, self.dim, k, chunk)
        if need < 0:
            ffi.check(int(need), name + "_workspace")
        work = self._work.get((B, k, path))
        if work is None or work.numel() < need:
            work = self._work[(B, k, path)] = torch.empty(int(need), dtype=torch.uint8, device=t.device)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(getattr(ffi.lib, name)(t.data_ptr(), self.dim, B, self._buf.data_ptr(), self.pitch, self._n, self.dim, k,
                                         int(chunk), scores.data_ptr(), indices.data_ptr(), work.data_ptr(), work.numel(), st), name)
        return Matches(Tensor(indices), Tensor(scores))

    # -- the exact search of a row range, and the join of matches (csrc/embed_merge.hip) ---------------------------
    def _range_args(self, k, start, stop, method, what="Gallery.search_range"):
        """every ``ValueError`` of ``search_range`` about ``k``, the range and ``method``; returns (start, rows, the ``k`` the
        search runs for -- ``min(k, rows)`` --, its path; None for an empty range).  No device work."""
        from ..engine import ffi
        if not _is_int(k):
            raise ValueError(f"{what}: k must be an integer, got {k!r}")
        if method not in _METHODS:
            raise ValueError(f"{what}: method = {method!r}, must be one of {', '.join(map(repr, _METHODS))}")
        if stop is None:
            stop = self._n
        if not _is_int(start) or not _is_int(stop):
            raise ValueError(f"{what}: start and stop must be integers (stop may be None: len), got {start!r} and {stop!r}")
        if not 0 <= start <= stop <= self._n:
            raise ValueError(f"{what}: rows [{start}, {stop}): 0 <= start <= stop <= len = {self._n} must hold")
        if k < 1 or k > ffi.EMBED_WIDE_MAX_K:
            raise ValueError(f"{what}: k = {k}, must be in [1, TFIMM_EMBED_WIDE_MAX_K = {ffi.EMBED_WIDE_MAX_K}] (it may exceed the "
                             f"rows of the range: the slots behind them hold -1 / -inf)")
        rows = int(stop) - int(start)
        ks = min(int(k), rows)
        if not rows:
            return int(start), 0, 0, None
        try:
            path = self._route(ks, method)                     # ks <= rows <= len: the width limits of the route remain
        except ValueError as e:
            raise ValueError(str(e).replace("Gallery.search", what)) from None
        return int(start), rows, ks, path

    def _range_launch(self, t, ks: int, start: int, rows: int, path: str):
        """the exact search of device queries ``t`` float32 (B, dim), B >= 1, among rows [start, start + rows) for ``ks <=
        rows`` neighbours by ``path`` -> (indices, scores) torch tensors (B, ks); the indices count from ``start``.  The
        existing entry points on the gallery's buffer at a row offset: ``pitch`` is a multiple of 8 elements, so the rows stay
        16-byte aligned.  Two launches on the current stream."""
        import torch
        from ..engine import ffi
        B = int(t.shape[0])
        scores = torch.empty((B, ks), dtype=torch.float32, device=t.device)
        indices = torch.empty((B, ks), dtype=torch.int32, device=t.device)
        name = "tfimm_hip_embed_search" if path == "list" else "tfimm_hip_embed_search_wide"
        need = getattr(ffi.lib, name + "_workspace")(B, rows, self.dim, ks, 0)
        if need < 0:
            ffi.check(int(need), name + "_workspace")
        # an entry of its own: a whole-gallery search that outgrows its workspace replaces that tensor, and a captured graph of
        # this search must not hold the address of a workspace another search can free
        work = self._work.get((B, ks, path, "range"))
        if work is None or work.numel() < need:
            work = self._work[(B, ks, path, "range")] = torch.empty(int(need), dtype=torch.uint8, device=t.device)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(getattr(ffi.lib, name)(t.data_ptr(), int(t.stride(0)), B, self._buf.data_ptr() + 2 * start * self.pitch, self.pitch,
                                         rows, self.dim, ks, 0, scores.data_ptr(), indices.data_ptr(), work.data_ptr(),
                                         work.numel(), st), name)
        return indices, scores

    def search_range(self, q, k: int = 5, start: int = 0, stop=None, method: str = "auto") -> Matches:
        """``search`` among the rows ``[start, stop)`` only (``stop=None``: ``len``): ``Matches`` whose indices are the
        gallery's own numbers, whose scores have the bits ``search`` gives for those rows, in ``search``'s order.  ``k <= 256``
        may exceed the rows of the range: the search runs for ``min(k, rows)`` and the slots behind hold index -1 and score
        -inf; an empty range gives nothing else and launches no search.  ``method`` and the width limits are those of
        ``search_with``, applied to ``min(k, rows)``.  The search's two launches on the gallery's buffer at a row offset, then
        tfimm_hip_matches_merge with one set, which adds ``start`` and fills; nothing goes to the host.  With ``merge_matches``
        this searches a gallery in pieces; ``GalleryIndex.search_live`` searches the rows an index does not hold with it."""
        import torch
        from ..engine import ffi
        what = "Gallery.search_range"
        start, rows, ks, path = self._range_args(k, start, stop, method, what)
        t = self._upload_rows(self._check_rows(q, "search_range")).contiguous()
        B, k = int(t.shape[0]), int(k)
        if B > ffi.EMBED_MAX_B:
            raise ValueError(f"{what}: {B} queries, at most TFIMM_EMBED_MAX_B = {ffi.EMBED_MAX_B} per call")
        if B == 0 or not rows:
            return Matches(Tensor(torch.full((B, k), -1, dtype=torch.int32, device=t.device)),
                           Tensor(torch.full((B, k), float("-inf"), dtype=torch.float32, device=t.device)))
        i, s = self._range_launch(t, ks, start, rows, path)
        indices, scores = _merge_launch([(i, s, start)], k)
        return Matches(Tensor(indices), Tensor(scores))

    # -- the coarse-to-fine search: fp8 scan, exact bf16 rerank (csrc/embed_coarse.hip) ---------------------------
    @property
    def coarse(self) -> bool:
        """whether the rows have an fp8 copy (``build_coarse``), which ``search_coarse`` scans"""
        return self._coarse

    def _grow_coarse(self) -> None:
        """codes and exponents for ``capacity`` rows; those of the first ``len`` rows are kept"""
        import torch
        if self._buf is None or (self._codes is not None and self._codes.shape[0] >= self._capacity):
            return
        codes = torch.zeros((self._capacity, self.dim), dtype=torch.uint8, device=self._buf.device)
        exps = torch.zeros(self._capacity, dtype=torch.int8, device=self._buf.device)
        if self._codes is not None and self._n:
            codes[:self._n].copy_(self._codes[:self._n])
            exps[:self._n].copy_(self._exps[:self._n])
        self._codes, self._exps = codes, exps

    def _quantize(self, first: int, n: int) -> None:
        """tfimm_hip_embed_quantize_rows of rows ``first .. first + n`` on the current stream; no synchronisation"""
        import torch
        from ..engine import ffi
        if not n:
            return
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_embed_quantize_rows(self._buf.data_ptr() + 2 * first * self.pitch, self.pitch, n, self.dim,
                                                        self._codes.data_ptr() + first * self.dim, self.dim,
                                                        self._exps.data_ptr() + first, st), "tfimm_hip_embed_quantize_rows")

    def build_coarse(self) -> None:
        """Give the gallery an fp8 copy of its rows for ``search_coarse``: per row one power-of-two scale (int8) and ``dim``
        OCP e4m3fn codes (tfimm_hip_embed_quantize_rows), ``dim + 1`` bytes next to the ``2 dim`` of the bf16 row.  From then
        on ``add`` quantises the rows it appends.  Calling it again quantises every row anew.  One launch on the current
        stream, no synchronisation; ``search`` and everything else are untouched."""
        self._coarse = True
        self._codes = self._exps = None
        self._grow_coarse()
        if self._buf is not None:
            self._quantize(0, self._n)

    def _coarse_args(self, k, candidates):
        """every ``ValueError`` of ``search_coarse`` about the gallery, ``k`` and ``candidates``; returns ``candidates``
        resolved.  No device work."""
        from ..engine import ffi
        what = "Gallery.search_coarse"
        if not self._coarse:
            raise ValueError(f"{what}: this gallery has no coarse copy: call build_coarse() first")
        if not _is_int(k):
            raise ValueError(f"{what}: k must be an integer, got {k!r}")
        if candidates is not None and not _is_int(candidates):
            raise ValueError(f"{what}: candidates must be an integer or None, got {candidates!r}")
        most = int(ffi.lib.tfimm_hip_embed_search_coarse_max_candidates(self.dim))
        c = min(max(4 * int(k), 32), most, self._n) if candidates is None else int(candidates)
        if c > most:
            raise ValueError(f"{what}: candidates = {c}: rows of dim {self.dim} allow candidates <= {most} "
                             f"(tfimm_hip_embed_search_coarse_max_candidates)")
        if c > self._n:
            raise ValueError(f"{what}: candidates = {c}, must be in [1, len = {self._n}]")
        if k < 1 or k > c:
            raise ValueError(f"{what}: k = {k}, must be in [1, candidates = {c}]")
        return c

    def search_coarse(self, q, k: int = 5, candidates=None, chunk: int = 0) -> Matches:
        """``Matches(indices, scores)`` as ``search`` gives them, by a coarse-to-fine search: every row is scanned as fp8 codes
        (``build_coarse``), the ``candidates`` rows with the largest coarse keys per query are scored exactly as ``search``
        scores them, and the ``k`` best of those are returned, score descending, equal scores by ascending row.  Every
        returned score has the bits ``search`` gives for that row; where the candidates contain the true top ``k`` -- with
        ``candidates = 4 k`` on random data always, on tightly clustered data not always -- the whole result
        is bit-equal.  ``candidates=None`` means ``min(max(4 k, 32), max_candidates(dim), len)``; at most
        ``tfimm_hip_embed_search_coarse_max_candidates(dim)`` (256, 254 at ``dim = 2048``).  Three launches on the current
        stream; the result does not depend on ``chunk``.  ``vote`` takes the matches as it takes those of ``search``."""
        import torch
        from ..engine import ffi
        c = self._coarse_args(k, candidates)
        t = self._rows(q, "search_coarse").contiguous()
        B, k = int(t.shape[0]), int(k)
        if B > ffi.EMBED_MAX_B:
            raise ValueError(f"Gallery.search_coarse: {B} queries, at most TFIMM_EMBED_MAX_B = {ffi.EMBED_MAX_B} per call")
        scores = torch.empty((B, k), dtype=torch.float32, device=t.device)
        indices = torch.empty((B, k), dtype=torch.int32, device=t.device)
        if B == 0:
            return Matches(Tensor(indices), Tensor(scores))
        name = "tfimm_hip_embed_search_coarse"
        need = ffi.lib.tfimm_hip_embed_search_coarse_workspace(B, self._n, self.dim, k, c, chunk)
        if need < 0:
            ffi.check(int(need), name + "_workspace")
        work = self._work_coarse.get((B, k, c))
        if work is None or work.numel() < need:
            work = self._work_coarse[(B, k, c)] = torch.empty(int(need), dtype=torch.uint8, device=t.device)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_embed_search_coarse(t.data_ptr(), self.dim, B, self._buf.data_ptr(), self.pitch,
                                                        self._codes.data_ptr(), self.dim, self._exps.data_ptr(), self._n, self.dim,
                                                        k, c, int(chunk), scores.data_ptr(), indices.data_ptr(), work.data_ptr(),
                                                        work.numel(), st), name)
        return Matches(Tensor(indices), Tensor(scores))

    # -- the kNN end: matches -> classes (csrc/knn.hip) ----------------------------------------------------------------------
    @staticmethod
    def _vote_args(what, temperature, top, reduce):
        """(inv_temperature, reduce id) of checked arguments"""
        from ..engine import ffi
        if reduce not in _REDUCE:
            raise ValueError(f"{what}: reduce = {reduce!r}, must be 'sum' or 'max'")
        if not _is_int(top) or not 1 <= top <= ffi.KNN_MAX_TOP:
            raise ValueError(f"{what}: top = {top!r}, must be an integer in [1, TFIMM_KNN_MAX_TOP = {ffi.KNN_MAX_TOP}]")
        inv_t = 0.0                                      # temperature=None: every weight is 1, the majority vote
        if reduce == "sum" and temperature is not None:
            ok = not isinstance(temperature, bool) and isinstance(temperature, (int, float, np.integer, np.floating))
            if ok:
                with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
                    inv_t = float(np.float32(1.0) / np.float32(temperature))
            if not ok or not temperature > 0 or not np.isfinite(inv_t):
                raise ValueError(f"{what}: temperature = {temperature!r}, must be a positive number whose inverse is a finite "
                                 f"float32, or None for the majority vote")
        return inv_t, _REDUCE.index(reduce)

    def _knn_k(self, what, k, exclude) -> int:
        """the ``k`` the search is asked for: one more with ``exclude``, whose row takes a place among the matches"""
        from ..engine import ffi
        if not _is_int(k):
            raise ValueError(f"{what}: k must be an integer, got {k!r}")
        extra = 0 if exclude is None else 1
        if k < 1 or k + extra > ffi.EMBED_MAX_K or k + extra > self._n:
            raise ValueError(f"{what}: k = {k}{' (+ 1 for the excluded row)' if extra else ''}, must be in [1, min(len = {self._n}, "
                             f"TFIMM_EMBED_MAX_K = {ffi.EMBED_MAX_K}){' - 1' if extra else ''}]")
        return int(k) + extra

    @staticmethod
    def _exclude(exclude, batch, what):
        if exclude is None:
            return None
        from .meter import _labels
        try:
            return _labels(exclude, batch, what)
        except ValueError as e:
            raise ValueError(str(e).replace("labels", "exclude")) from None

    def _matches(self, matches, what):
        """(indices, scores) of a ``Matches`` as the int32 / float32 device tensors (B, k) they must be"""
        import torch
        from ..engine import ffi
        try:
            i, s = (m.torch() if isinstance(m, Tensor) else m for m in matches)
            ok = isinstance(i, torch.Tensor) and isinstance(s, torch.Tensor)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{what}: matches must be the Matches(indices, scores) of Gallery.search")
        if i.dtype != torch.int32 or s.dtype != torch.float32 or i.ndim != 2 or i.shape != s.shape:
            raise ValueError(f"{what}: matches: expected int32 indices and float32 scores of one shape (B, k), got {i.dtype} "
                             f"{tuple(i.shape)} and {s.dtype} {tuple(s.shape)}")
        if not 1 <= i.shape[1] <= ffi.KNN_MAX_K:
            raise ValueError(f"{what}: matches with k = {i.shape[1]}, must be in [1, TFIMM_KNN_MAX_K = {ffi.KNN_MAX_K}]")
        if not (i.is_cuda and s.is_cuda):
            raise ValueError(f"{what}: matches must be on the device (what Gallery.search returns)")
        return i.contiguous(), s.contiguous()

    def _launch_vote(self, i, s, up_exclude, inv_t, reduce, top) -> Votes:
        """tfimm_hip_knn_vote on the current stream, behind whatever produced the matches there; no synchronisation"""
        import torch
        from ..engine import ffi
        B, k = int(i.shape[0]), int(i.shape[1])
        dev = i.device
        classes = torch.empty((B, top), dtype=torch.int32, device=dev)
        values = torch.empty((B, top), dtype=torch.float32, device=dev)
        counts = torch.empty((B, top), dtype=torch.int32, device=dev)
        total = torch.empty(B, dtype=torch.float32, device=dev)
        if B:
            ex = None if up_exclude is None else up_exclude()
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            ffi.check(ffi.lib.tfimm_hip_knn_vote(i.data_ptr(), s.data_ptr(), k, B, k, self._lab.data_ptr(), self._n,
                                                 None if ex is None else ex.data_ptr(), inv_t, reduce, top, classes.data_ptr(),
                                                 values.data_ptr(), counts.data_ptr(), total.data_ptr(), st), "tfimm_hip_knn_vote")
        return Votes(Tensor(classes), Tensor(values), Tensor(counts), Tensor(total))

    def vote(self, matches, temperature=0.07, top: int = 5, reduce: str = "sum", exclude=None) -> Votes:
        """``Votes(classes, values, counts, total)`` of the ``Matches`` of a search of this gallery: per query the ``top``
        classes among the labels of its matches.  ``reduce="sum"``: a vote weighted by ``exp((score - best) / temperature)``
        (``temperature=None``: every match counts 1, the majority vote); ``values`` are the classes' sums, ``total`` the sum
        over all matches, ``values / total`` the shares.  ``reduce="max"``: the best row per identity -- ``values`` are raw
        scores, ``temperature`` is ignored; the classes are exactly the top distinct identities of the whole gallery (an
        identity that is missing has its best row below the k-th score).  ``counts``: the matches of each class.  Order: value
        descending, equal values by ascending class; slots beyond the distinct classes hold (-1, 0, 0).  Rows labelled -1
        never vote, nor does ``exclude[b]`` -- an int vector (B,), the gallery row query ``b`` must not meet (itself, in a
        leave-one-out evaluation; -1: none).  One launch (tfimm_hip_knn_vote) on the current stream, no synchronisation.
        ``Matches`` of more than 64 columns (``TFIMM_KNN_MAX_K``) -- ``search`` returns up to 256 -- are refused."""
        what = "Gallery.vote"
        self._need_labels(what)
        inv_t, red = self._vote_args(what, temperature, top, reduce)
        if not self._n:
            raise ValueError(f"{what}: the gallery is empty")
        i, s = self._matches(matches, what)
        up_ex = self._exclude(exclude, int(i.shape[0]), what)
        return self._launch_vote(i, s, up_ex, inv_t, red, int(top))

    def _plan_classify(self, what, batch, k, temperature, top, reduce, exclude, chunk=0):
        """every ``ValueError`` of ``classify`` for a batch of ``batch`` queries; returns the device part, ``run(q)``"""
        self._need_labels(what)
        inv_t, red = self._vote_args(what, temperature, top, reduce)
        ks = self._knn_k(what, k, exclude)
        up_ex = self._exclude(exclude, batch, what)

        def run(q) -> Votes:
            m = self.search(q, ks, chunk)
            return self._launch_vote(m.indices.torch(), m.scores.torch(), up_ex, inv_t, red, int(top))
        return run

    def classify(self, q, k: int = 20, temperature=0.07, top: int = 5, reduce: str = "sum", exclude=None, chunk: int = 0) -> Votes:
        """``vote(search(q, k), ...)``: the classes of float32 queries ``q`` (B, dim) from their ``k`` nearest labelled rows,
        three launches on the current stream and nothing on the host.  With ``exclude`` the search asks for ``k + 1`` rows
        (the excluded one takes a place), so ``k <= 63`` and ``k + 1 <= len``: ``classify(rows, exclude=arange(len))``
        evaluates a gallery against itself, leave-one-out."""
        t = self._check_rows(q, "classify")
        return self._plan_classify("Gallery.classify", int(t.shape[0]), k, temperature, top, reduce, exclude, chunk)(q)

    def _plan_evaluate(self, what, batch, labels, k, temperature, meter, nb_classes, exclude):
        """every ``ValueError`` of ``evaluate`` for a batch of ``batch`` queries; returns the device part, ``run(q)``"""
        from .meter import Meter, Scores, _labels
        self._need_labels(what)
        if meter is not None and not isinstance(meter, Meter):
            raise ValueError(f"{what}: meter must be a tfimm.Meter, got {type(meter).__name__}")
        if meter is None and nb_classes is None:
            raise ValueError(f"{what}: nb_classes is needed: pass it, or a meter that knows it")
        if nb_classes is not None and (not _is_int(nb_classes) or not 1 <= nb_classes <= 2 ** 31 - 1):
            raise ValueError(f"{what}: nb_classes = {nb_classes!r}, must be an integer in [1, 2^31 - 1]")
        if meter is not None and nb_classes is not None and meter.nb_classes != nb_classes:
            raise ValueError(f"{what}: the meter counts {meter.nb_classes} classes, nb_classes = {nb_classes}")
        n = int(meter.nb_classes if meter is not None else nb_classes)
        inv_t, _ = self._vote_args(what, temperature, 1, "sum")
        ks = self._knn_k(what, k, exclude)
        up_labels = _labels(labels, batch, what)
        up_ex = self._exclude(exclude, batch, what)

        def run(q) -> Scores:
            import torch
            from ..engine import ffi
            m = self.search(q, ks)
            i, s = m.indices.torch(), m.scores.torch()
            B, dev = int(i.shape[0]), i.device
            loss = torch.empty(B, dtype=torch.float32, device=dev)
            rank = torch.empty(B, dtype=torch.int32, device=dev)
            pred = torch.empty(B, dtype=torch.int32, device=dev)
            prob = torch.empty(B, dtype=torch.float32, device=dev)
            if B:
                y = up_labels()
                ex = None if up_ex is None else up_ex()
                acc = (None, None, None)
                if meter is not None:
                    if meter._buf is None:
                        meter._buf = torch.zeros(meter._layout()[2], dtype=torch.int64, device=dev)
                    acc = meter._views()
                ptr = [None if t is None else t.data_ptr() for t in acc]
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                ffi.check(ffi.lib.tfimm_hip_knn_score(i.data_ptr(), s.data_ptr(), ks, B, ks, self._lab.data_ptr(), self._n,
                                                      None if ex is None else ex.data_ptr(), inv_t, n, y.data_ptr(),
                                                      loss.data_ptr(), rank.data_ptr(), pred.data_ptr(), prob.data_ptr(),
                                                      ptr[0], ptr[1], ptr[2], st), "tfimm_hip_knn_score")
            return Scores(Tensor(loss), Tensor(rank), Tensor(pred), Tensor(prob))
        return run

    def evaluate(self, q, labels, k: int = 20, temperature=0.07, meter=None, nb_classes=None, exclude=None):
        """How good is the embedding: the weighted vote of ``classify(q, k, temperature)`` scored against the true
        ``labels`` (B,) -- ``Scores(loss, rank, pred, prob)`` as ``tfimm.score`` gives them for logits, with the vote vector
        in their place: ``pred`` the winning class, ``rank`` the true class's position among all ``nb_classes`` (an unvoted
        class holds 0 and ties by ascending class), ``prob`` its share of the vote, ``loss = -log(prob)`` (inf when nobody
        voted for it: the meter counts such a row in ``loss_excluded``).  With a ``tfimm.Meter`` the batch is added to it on
        the device -- the same meter ``tfimm.score`` feeds; ``nb_classes`` comes from it, or from the argument.  A label of
        -1 is not scored; gallery rows whose label is not below ``nb_classes`` do not vote.  ``exclude`` as in ``classify``.
        Three launches on the current stream (tfimm_hip_knn_score behind the search), no synchronisation."""
        t = self._check_rows(q, "evaluate")
        return self._plan_evaluate("Gallery.evaluate", int(t.shape[0]), labels, k, temperature, meter, nb_classes, exclude)(q)

    # -- the cluster end: rows -> groups (csrc/cluster.hip) ------------------------------------------------------------------
    def set_labels(self, labels) -> None:
        """Replace the label of every row: ``labels`` (len,), in the forms ``add`` takes, on either side (host labels below -1
        are refused, device labels are not looked at).  Makes an unlabelled gallery a labelled one:
        ``gallery.set_labels(clusters.assignment)`` lets ``vote`` / ``classify`` / ``evaluate`` answer with clusters."""
        import torch
        up = _row_labels(labels, self._n, "Gallery.set_labels")
        if self._n:
            lab = up()
            if self._lab is None or self._lab.shape[0] < self._capacity:
                self._lab = torch.full((self._capacity,), -1, dtype=torch.int32, device=lab.device)
            self._lab[:self._n].copy_(lab)
        self._labelled = True

    @classmethod
    def _of_rows(cls, dim, rows, labels):
        """a labelled gallery over float32 device rows (n, dim) -- rounded to bf16, nearest even -- and int32 labels (n,)"""
        import torch
        g = cls(dim)
        n = int(rows.shape[0])
        g._buf = torch.zeros((n, g.pitch), dtype=torch.bfloat16, device=rows.device)
        g._buf[:, :dim].copy_(rows)
        g._lab = labels.to(torch.int32).contiguous()
        g._n = g._capacity = n
        g._labelled = True
        return g

    def _check_centroids(self, what, centroids) -> None:
        from ..engine import ffi
        if not isinstance(centroids, Gallery):
            raise ValueError(f"{what}: centroids must be a Gallery, got {type(centroids).__name__}")
        if centroids.dim != self.dim:
            raise ValueError(f"{what}: centroids of dim {centroids.dim}, this gallery holds rows of {self.dim}")
        if not 1 <= len(centroids) <= ffi.CLUSTER_MAX_C:
            raise ValueError(f"{what}: {len(centroids)} centroids, must be in [1, TFIMM_CLUSTER_MAX_C = {ffi.CLUSTER_MAX_C}] "
                             f"(an empty Gallery holds none)")
        if not self._n:
            raise ValueError(f"{what}: the gallery is empty")

    def _launch_assign(self, cbuf, cpitch: int, nc: int):
        """tfimm_hip_cluster_assign of every row against the bf16 centroids ``cbuf`` (nc, cpitch) on the current stream ->
        (int32 (len,), float32 (len,)) torch tensors; no synchronisation"""
        import torch
        from ..engine import ffi
        dev = self._buf.device
        clusters = torch.empty(self._n, dtype=torch.int32, device=dev)
        scores = torch.empty(self._n, dtype=torch.float32, device=dev)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_cluster_assign(self._buf.data_ptr(), self.pitch, self._n, cbuf.data_ptr(), cpitch, nc, self.dim,
                                                   clusters.data_ptr(), scores.data_ptr(), st), "tfimm_hip_cluster_assign")
        return clusters, scores

    def assign(self, centroids) -> "Assigned":
        """``Assigned(clusters, scores)``: for every row the row of ``centroids`` -- a ``Gallery`` of the same ``dim`` -- with
        the largest inner product (of equal scores the lowest) and that score, two ``Tensor`` (len,), int32 / float32.  One
        launch (tfimm_hip_cluster_assign) on the current stream, no synchronisation; the (len, centroids) score matrix never
        exists."""
        self._check_centroids("Gallery.assign", centroids)
        a, s = self._launch_assign(centroids._buf, centroids.pitch, len(centroids))
        return Assigned(Tensor(a), Tensor(s))

    def _segment_means(self, groups, nb: int):
        """the float32 mean (nb, dim) and the int32 count (nb,) of the rows of every group: ``groups`` int32 (len,) on the
        device, a row whose group is outside [0, nb) belongs to none.  The CSR form is plumbing -- a stable sort of the groups
        and ``searchsorted`` by ``torch`` on the device --, the means are tfimm_hip_segment_mean; no synchronisation."""
        import torch
        from ..engine import ffi
        dev = groups.device
        ordered, order = torch.sort(groups, stable=True)
        offsets = torch.searchsorted(ordered, torch.arange(nb + 1, dtype=torch.int32, device=dev), out_int32=True).contiguous()
        rows = order.to(torch.int32).contiguous()
        need = ffi.lib.tfimm_hip_segment_mean_workspace(self._n, nb, self.dim)
        if need < 0:
            ffi.check(int(need), "tfimm_hip_segment_mean_workspace")
        work = self._work.get("segment_mean")
        if work is None or work.numel() < need:
            work = self._work["segment_mean"] = torch.empty(int(need), dtype=torch.uint8, device=dev)
        mean = torch.empty((nb, self.dim), dtype=torch.float32, device=dev)
        counts = torch.empty(nb, dtype=torch.int32, device=dev)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_segment_mean(self._buf.data_ptr(), self.pitch, self._n, self.dim, rows.data_ptr(), self._n,
                                                 offsets.data_ptr(), nb, mean.data_ptr(), self.dim, counts.data_ptr(),
                                                 work.data_ptr(), work.numel(), st), "tfimm_hip_segment_mean")
        return mean, counts

    def _normalize(self, x):
        """tfimm_hip_l2_normalize of the float32 device rows ``x`` (n, dim), in place"""
        import torch
        from ..engine import ffi
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_l2_normalize(x.data_ptr(), self.dim, int(x.shape[0]), self.dim, x.data_ptr(), self.dim, st),
                  "tfimm_hip_l2_normalize")
        return x

    def prototypes(self, nb_classes=None, normalize: bool = True) -> "Gallery":
        """One row per class of a labelled gallery: a new labelled ``Gallery`` of ``nb_classes`` rows, row ``c`` the mean of
        the rows labelled ``c`` (tfimm_hip_segment_mean), L2-normalised if asked (tfimm_hip_l2_normalize), rounded to bf16 and
        labelled ``c``.  A class without rows gets a zero row labelled -1, so it never votes; labels that are -1 or
        ``>= nb_classes`` belong to no class.  ``nb_classes=None`` reads the largest label from the device (the one
        synchronisation); given ``nb_classes`` there is none.  ``prototypes().classify(q, k=1)`` and ``.search(q, 1)`` are the
        nearest-class-mean classifier: a gallery of ``nb_classes`` rows at ``k = 1``, where the search is at its best."""
        import torch
        what = "Gallery.prototypes"
        self._need_labels(what)
        if nb_classes is not None and (not _is_int(nb_classes) or not 1 <= nb_classes <= 2 ** 31 - 2):
            raise ValueError(f"{what}: nb_classes = {nb_classes!r}, must be an integer in [1, 2^31 - 2] or None")
        if not self._n:
            raise ValueError(f"{what}: the gallery is empty")
        lab = self._lab[:self._n]
        if nb_classes is None:
            nb_classes = int(lab.max().item()) + 1
            if nb_classes < 1:
                raise ValueError(f"{what}: nb_classes: no row of this gallery carries a class (every label is -1)")
        nb = int(nb_classes)
        mean, counts = self._segment_means(lab, nb)
        if normalize:
            self._normalize(mean)
        classes = torch.arange(nb, dtype=torch.int32, device=mean.device)
        return Gallery._of_rows(self.dim, mean, torch.where(counts > 0, classes, torch.full_like(classes, -1)))

    def _plan_kmeans(self, n_clusters, iters, init, seed):
        """every ``ValueError`` of ``kmeans``; returns the initial centroids as ("rows", int64 indices), ("values", float32
        (n_clusters, dim) array or tensor) or ("gallery", a ``Gallery`` of n_clusters rows)"""
        import torch
        from ..engine import ffi
        what = "Gallery.kmeans"
        if not self._n:
            raise ValueError(f"{what}: the gallery is empty")
        top = min(self._n, ffi.CLUSTER_MAX_C)
        if not _is_int(n_clusters) or not 1 <= n_clusters <= top:
            raise ValueError(f"{what}: n_clusters = {n_clusters!r}, must be an integer in [1, min(len = {self._n}, "
                             f"TFIMM_CLUSTER_MAX_C = {ffi.CLUSTER_MAX_C})]")
        if not _is_int(iters) or iters < 0:
            raise ValueError(f"{what}: iters = {iters!r}, must be an integer that is not negative")
        k = int(n_clusters)
        if init is None:
            return "rows", np.random.default_rng(seed).choice(self._n, k, replace=False).astype(np.int64)
        if isinstance(init, Gallery):
            if init.dim != self.dim or len(init) != k:
                raise ValueError(f"{what}: init: a Gallery of {len(init)} rows of dim {init.dim}, expected {k} rows of {self.dim}")
            return "gallery", init
        t = init.torch() if isinstance(init, Tensor) else init
        if not isinstance(t, torch.Tensor):
            t = np.asarray(t)
        kind = str(t.dtype).replace("torch.", "")
        if kind.startswith(("int", "uint")):
            a = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
            if a.shape != (k,):
                raise ValueError(f"{what}: init: {k} row indices expected, got shape {tuple(a.shape)}")
            a = a.astype(np.int64)
            if a.min() < 0 or a.max() >= self._n:
                raise ValueError(f"{what}: init: row indices must be in [0, len = {self._n}), got values in [{a.min()}, {a.max()}]")
            if len(np.unique(a)) != k:
                raise ValueError(f"{what}: init: row indices must be distinct")
            return "rows", a
        if kind != "float32":
            raise ValueError(f"{what}: init: expected row indices (integers) or float32 values, got {t.dtype}")
        if t.ndim != 2 or tuple(t.shape) != (k, self.dim):
            raise ValueError(f"{what}: init: expected shape ({k}, {self.dim}), got {tuple(t.shape)}")
        return "values", t

    def kmeans(self, n_clusters: int, iters: int = 10, init=None, seed: int = 0) -> "Clusters":
        """Spherical k-means -- Lloyd iterations on the inner product -- over the rows, on the device:
        ``Clusters(centroids, assignment, scores, counts, moved)``.  Initial centroids: ``init=None`` takes the rows
        ``np.random.default_rng(seed).choice(len, n_clusters, replace=False)``; ``init`` may be an integer array of
        ``n_clusters`` distinct row indices, or float32 (n_clusters, dim) values as an array, a ``Tensor`` or a ``Gallery``;
        they are L2-normalised and rounded to bf16 like all later ones.  An iteration is assign (tfimm_hip_cluster_assign),
        the CSR form of the groups (``torch``), their means (tfimm_hip_segment_mean), tfimm_hip_l2_normalize, bf16; an empty
        cluster keeps its previous centroid.  After ``iters`` updates one more assign runs, so that ``assignment`` / ``scores``
        / ``counts`` (int32, float32, int32 ``Tensor``) belong to the returned ``centroids`` -- a labelled ``Gallery`` with
        label ``j`` on row ``j`` -- : ``iters + 1`` assign launches, ``iters=0`` only assigns.  ``moved``: int32 ``Tensor``
        (iters,), the rows whose assignment changed between consecutive assign passes.  Nothing synchronises with the host:
        callers read ``moved`` if they want a stopping rule."""
        import torch
        how, start = self._plan_kmeans(n_clusters, iters, init, seed)
        k, dev = int(n_clusters), self._buf.device
        if how == "rows":
            x = self._buf[torch.from_numpy(start).to(dev), :self.dim].float()
        elif how == "gallery":
            x = start._buf[:k, :self.dim].to(dev).float()
        else:
            x = self._upload_rows(start).to(dev).float()
        cen = torch.zeros((k, self.pitch), dtype=torch.bfloat16, device=dev)
        cen[:, :self.dim].copy_(self._normalize(x.contiguous().clone()))
        moved = torch.zeros(int(iters), dtype=torch.int32, device=dev)
        a, s = self._launch_assign(cen, self.pitch, k)
        for it in range(int(iters)):
            mean, counts = self._segment_means(a, k)
            new = self._normalize(mean).to(torch.bfloat16)
            cen[:, :self.dim] = torch.where((counts > 0)[:, None], new, cen[:, :self.dim])
            a2, s = self._launch_assign(cen, self.pitch, k)
            moved[it] = (a2 != a).sum()
            a = a2
        counts = torch.zeros(k, dtype=torch.int32, device=dev).scatter_add_(0, a.long(), torch.ones_like(a))
        centroids = Gallery._of_rows(self.dim, cen[:, :self.dim].float(), torch.arange(k, dtype=torch.int32, device=dev))
        return Clusters(centroids, Tensor(a), Tensor(s), Tensor(counts), Tensor(moved))

    # -- the inverted-list index over the k-means lists (gallery_index.py; csrc/embed_lists.hip) ----------------------
    def build_index(self, n_lists=None, iters: int = 10, init=None, seed: int = 0, clusters=None):
        """A ``tfimm.GalleryIndex`` over the rows the gallery holds now: ``kmeans(n_lists, iters, init, seed)`` groups them --
        ``n_lists=None`` means ``round(sqrt(len))``, clamped to [1, TFIMM_CLUSTER_MAX_C]; or pass the ``Clusters`` of an earlier
        ``kmeans`` as ``clusters`` --, and every group becomes an inverted list: a stable sort of the assignment,
        ``searchsorted`` for the offsets and a gather of the rows, by ``torch`` on the device.  The index owns a list-ordered
        copy of the bf16 rows, so it DOUBLES the gallery's memory.  One host synchronisation: the length of the longest list,
        from which the search's workgroups per list are derived.  The index is a snapshot: rows added later are not in it
        (``index.stale``) until a new build.  ``search``, ``classify`` and ``evaluate`` of the gallery are untouched and never
        take the index: ``index.search(q, k, nprobe)`` does."""
        from .gallery_index import build_index
        return build_index(self, n_lists, iters, init, seed, clusters)
