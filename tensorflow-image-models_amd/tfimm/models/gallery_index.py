"""``GalleryIndex``: an inverted-list index over a ``Gallery`` -- the rows grouped by their best k-means centroid, and a search
that scores only the lists a query probes (tfimm_hip_embed_search_lists, csrc/embed_lists.hip).  Every
search path of ``Gallery`` reads the whole gallery; this one reads ``nprobe`` of ``n_lists`` lists, and pays with recall: a row
whose list is not probed is not found.  The rule is restated on the CPU in tests/index_ref.py.  ``search_with`` chooses the
first pass -- one query per workgroup, or the queries of a list grouped into MFMA tiles (tfimm_hip_embed_search_lists_grouped,
csrc/embed_lists_grouped.hip): the same bits --, and ``neighbours`` is the kNN graph of the indexed rows.  The
index follows a gallery that grows: ``search_live`` / ``classify_live`` search the probed lists AND every row
added since the build -- the exact search of that row range, joined by tfimm_hip_matches_merge (csrc/embed_merge.hip; the rule
is tests/live_ref.py) --, and ``absorb`` takes those rows into the lists without a k-means run."""
import ctypes as C
import math

import numpy as np

from .gallery import Clusters, Gallery, Matches, Votes, _is_int
from .model import Tensor

#: gallery rows per workgroup of the first pass that ``parts`` is derived from: the longest list is cut into about that many
ROWS_PER_PART = 2048

#: the first passes of ``GalleryIndex.search_with``: tfimm_hip_embed_search_lists_grouped and tfimm_hip_embed_search_lists
_METHODS = ("grouped", "single")


class GalleryIndex:
    """What ``gallery.build_index(...)`` returns: a SNAPSHOT of the gallery's first ``size`` rows as ``n_lists`` inverted
    lists.  The index owns a copy of the bf16 rows in list order (the gallery's memory, once more), the original row of every
    position (``ids``, ascending inside a list) and the lists' ``offsets``; ``centroids`` is the labelled ``Gallery`` of
    ``kmeans`` and ``counts`` the rows per list.  Rows added to the gallery later are not seen by ``search``, ``search_with``,
    ``classify`` and ``neighbours``: ``stale`` says that there are some, ``fresh`` how many.  ``search_live`` and
    ``classify_live`` see them -- they search the rows behind the snapshot exactly and merge --, ``absorb`` moves them into
    the lists (the centroids stay), and a new ``build_index`` clusters anew.  ``Gallery.search``, ``classify`` and
    ``evaluate`` never come here."""

    def __init__(self, gallery, clusters):
        cen = clusters.centroids
        assignment = clusters.assignment.torch() if isinstance(clusters.assignment, Tensor) else clusters.assignment
        self._gallery = gallery
        self.dim, self.pitch = gallery.dim, gallery.pitch
        self.n_lists = len(cen)
        self.centroids = cen
        self._lay(assignment)

    def _lay(self, assignment):
        """the lists of the gallery's rows as ``assignment`` (len,) groups them: what the constructor and ``absorb`` share"""
        import torch
        gallery, n, nl = self._gallery, len(self._gallery), self.n_lists
        self.size = n
        # plumbing, as Gallery._segment_means does it: a stable sort of the lists (rows ascend inside a list) and searchsorted
        ordered, order = torch.sort(assignment, stable=True)
        dev = ordered.device
        self._offsets = torch.searchsorted(ordered, torch.arange(nl + 1, dtype=torch.int32, device=dev), out_int32=True).contiguous()
        self._ids = order.to(torch.int32).contiguous()
        self._rows = gallery._buf[:n].index_select(0, order).contiguous()          # bf16 (size, pitch): the rows in list order
        self.counts = Tensor((self._offsets[1:] - self._offsets[:-1]).contiguous())
        longest = int(self.counts.torch().max().item())                              # the build's one synchronisation
        self.longest = longest
        self.parts = min(max(-(-longest // ROWS_PER_PART), 1), _ffi().EMBED_LISTS_MAX_PARTS)
        self._work = {}                                                              # (B, k, nprobe, parts) -> workspace (uint8); search_with: (method, B, ...)

    # -- what the index is ---------------------------------------------------------------------------------------------------
    @property
    def stale(self) -> bool:
        """whether the gallery has grown since the build: its later rows are not searched"""
        return len(self._gallery) != self.size

    @property
    def fresh(self) -> int:
        """the rows the gallery holds and the snapshot does not: ``len(gallery) - size``; ``search_live`` searches them
        exactly, ``absorb`` takes them into the lists"""
        return len(self._gallery) - self.size

    def lists(self):
        """``(ids, offsets)`` as numpy int32 arrays, (size,) and (n_lists + 1,): list ``l`` holds the original rows
        ``ids[offsets[l] : offsets[l + 1]]``, ascending (two device -> host copies)"""
        return self._ids.cpu().numpy(), self._offsets.cpu().numpy()

    # -- arguments: every ValueError before any device work ------------------------------------------------------------------------
    def _args(self, k, nprobe, parts=0, what="GalleryIndex.search"):
        """every ``ValueError`` of ``search`` about ``k``, ``nprobe`` and ``parts``; returns ``parts`` resolved.  No device work."""
        ffi = _ffi()
        if not _is_int(k):
            raise ValueError(f"{what}: k must be an integer, got {k!r}")
        if not _is_int(nprobe):
            raise ValueError(f"{what}: nprobe must be an integer, got {nprobe!r}")
        if not _is_int(parts):
            raise ValueError(f"{what}: parts must be an integer, got {parts!r}")
        if k < 1 or k > ffi.EMBED_WIDE_MAX_K:
            raise ValueError(f"{what}: k = {k}, must be in [1, TFIMM_EMBED_WIDE_MAX_K = {ffi.EMBED_WIDE_MAX_K}] (it may exceed the "
                             f"rows probed: the slots behind them hold -1 / -inf)")
        most = min(self.n_lists, ffi.EMBED_LISTS_MAX_PROBE)
        if nprobe < 1 or nprobe > most:
            raise ValueError(f"{what}: nprobe = {nprobe}, must be in [1, min(n_lists = {self.n_lists}, TFIMM_EMBED_LISTS_MAX_PROBE = "
                             f"{ffi.EMBED_LISTS_MAX_PROBE})]")
        try:
            self.centroids._route(int(nprobe))                 # the probe is a search of the centroids
        except ValueError as e:
            raise ValueError(f"{what}: nprobe = {nprobe}: the probe is centroids.search(q, nprobe): {e}") from None
        if parts < 0 or parts > ffi.EMBED_LISTS_MAX_PARTS:
            raise ValueError(f"{what}: parts = {parts}, must be 0 (derived from the longest list) or in [1, {ffi.EMBED_LISTS_MAX_PARTS}]")
        return int(parts) if parts else self.parts

    def _queries(self, q, what):
        try:
            t = self._gallery._check_rows(q, "search")
        except ValueError as e:
            raise ValueError(str(e).replace("Gallery.search", what)) from None
        if int(t.shape[0]) > _ffi().EMBED_LISTS_MAX_B:
            raise ValueError(f"{what}: {int(t.shape[0])} queries, at most {_ffi().EMBED_LISTS_MAX_B} per call")
        return t

    # -- the search ----------------------------------------------------------------------------------------------------------------
    def probe(self, q, nprobe: int = 8) -> Tensor:
        """int32 ``Tensor`` (B, nprobe): ``centroids.search(q, nprobe).indices`` -- per query the ``nprobe`` best lists by
        centroid score descending, equal scores by ascending list.  No kernel of its own."""
        self._args(1, nprobe, 0, "GalleryIndex.probe")
        return self.centroids.search(self._queries(q, "GalleryIndex.probe"), int(nprobe)).indices

    def search(self, q, k: int = 5, nprobe: int = 8, parts: int = 0) -> Matches:
        """``Matches(indices, scores)`` for float32 queries ``q`` (B, dim): per query the ``k`` best rows AMONG THE ``nprobe``
        LISTS whose centroids score best -- score descending, equal scores by ascending row, rows as the gallery numbers
        them, every score with the bits ``Gallery.search`` gives for that row.  A row in a list that is not probed is not
        found; with ``nprobe == n_lists`` the result is ``Gallery.search``'s.  ``k <= 256`` may exceed the rows probed: the
        slots behind them hold index -1 and score -inf.  ``1 <= nprobe <= min(n_lists, 256)``.  ``parts``: workgroups per
        list, 0 = derived at build time from the longest list (about 2048 rows each, at most 64); the result does not depend
        on it.  The probe's two launches and the search's two on the current stream; nothing goes to the host."""
        import torch
        ffi = _ffi()
        what = "GalleryIndex.search"
        parts = self._args(k, nprobe, parts, what)
        t = self._gallery._upload_rows(self._queries(q, what)).contiguous()
        B, k, nprobe = int(t.shape[0]), int(k), int(nprobe)
        scores = torch.empty((B, k), dtype=torch.float32, device=t.device)
        indices = torch.empty((B, k), dtype=torch.int32, device=t.device)
        if B == 0:
            return Matches(Tensor(indices), Tensor(scores))
        probes = self.centroids.search(t, nprobe).indices.torch()
        need = ffi.lib.tfimm_hip_embed_search_lists_workspace(B, self.size, self.dim, self.n_lists, nprobe, k, parts)
        if need < 0:
            ffi.check(int(need), "tfimm_hip_embed_search_lists_workspace")
        work = self._work.get((B, k, nprobe, parts))
        if work is None or work.numel() < need:
            work = self._work[(B, k, nprobe, parts)] = torch.empty(int(need), dtype=torch.uint8, device=t.device)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_embed_search_lists(t.data_ptr(), self.dim, B, self._rows.data_ptr(), self.pitch, self.size, self.dim,
                                                       self._ids.data_ptr(), self._offsets.data_ptr(), self.n_lists, probes.data_ptr(),
                                                       nprobe, nprobe, k, parts, scores.data_ptr(), indices.data_ptr(), work.data_ptr(),
                                                       work.numel(), st), "tfimm_hip_embed_search_lists")
        return Matches(Tensor(indices), Tensor(scores))

    def _method_args(self, k, nprobe, parts, method, what):
        """every ``ValueError`` of ``search_with`` / ``neighbours`` about ``k`` (as the search is asked for it), ``nprobe``,
        ``parts`` and ``method``; returns ``parts`` resolved.  No device work."""
        ffi = _ffi()
        if method not in _METHODS:
            raise ValueError(f"{what}: method = {method!r}, must be one of {', '.join(map(repr, _METHODS))}")
        parts = self._args(k, nprobe, parts, what)
        if method == "grouped":
            wide = int(ffi.lib.tfimm_hip_embed_search_wide_max_k(self.dim))  # 32 buffers share LDS with a query tile of this width
            if k > wide:
                raise ValueError(f"{what}: k = {k} with method='grouped': rows of dim {self.dim} allow "
                                 f"{'k <= ' + str(wide) if wide > 0 else 'no k'} on this path (tfimm_hip_embed_search_wide_max_k); "
                                 f"method='single' goes up to {ffi.EMBED_WIDE_MAX_K}")
        return parts

    def _launch(self, t, probes, k, nprobe, parts, method):
        """the search of device queries ``t`` float32 (B, dim), B >= 1, over ``probes`` int32 (B, nprobe) by ``method`` ->
        (indices, scores) torch tensors; the launches go on the current stream"""
        import torch
        ffi = _ffi()
        name = "tfimm_hip_embed_search_lists" + ("_grouped" if method == "grouped" else "")
        B = int(t.shape[0])
        scores = torch.empty((B, k), dtype=torch.float32, device=t.device)
        indices = torch.empty((B, k), dtype=torch.int32, device=t.device)
        need = getattr(ffi.lib, name + "_workspace")(B, self.size, self.dim, self.n_lists, nprobe, k, parts)
        if need < 0:
            ffi.check(int(need), name + "_workspace")
        work = self._work.get((method, B, k, nprobe, parts))
        if work is None or work.numel() < need:
            work = self._work[(method, B, k, nprobe, parts)] = torch.empty(int(need), dtype=torch.uint8, device=t.device)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(getattr(ffi.lib, name)(t.data_ptr(), int(t.stride(0)), B, self._rows.data_ptr(), self.pitch, self.size, self.dim,
                                         self._ids.data_ptr(), self._offsets.data_ptr(), self.n_lists, probes.data_ptr(), nprobe, nprobe,
                                         k, parts, scores.data_ptr(), indices.data_ptr(), work.data_ptr(), work.numel(), st), name)
        return indices, scores

    def search_with(self, q, k: int = 5, nprobe: int = 8, parts: int = 0, method: str = "grouped") -> Matches:
        """``search`` by a chosen first pass: the same ``Matches``, bit for bit.  ``method="single"`` is ``search``'s
        (tfimm_hip_embed_search_lists: one workgroup per query, probed list and part, so every query reads its lists on its
        own); ``"grouped"`` scores every probed list once for up to 32 of the queries that name it
        (tfimm_hip_embed_search_lists_grouped): fewer gallery bytes when the batch names a list many times
        (``B * nprobe`` well above ``n_lists``), more work per query when it does not.  ``"grouped"`` keeps 32 buffers in LDS:
        ``k <= tfimm_hip_embed_search_wide_max_k(dim)`` -- 256 up to dim 768, 254 at 1024, nothing at 2048.  There is no
        ``"auto"``: DESIGN.md 3.29 has the measurements one would be placed by.  The workspace is cached per
        ``(method, B, k, nprobe, parts)``."""
        import torch
        what = "GalleryIndex.search_with"
        parts = self._method_args(k, nprobe, parts, method, what)
        t = self._gallery._upload_rows(self._queries(q, what)).contiguous()
        B, k, nprobe = int(t.shape[0]), int(k), int(nprobe)
        if B == 0:
            return Matches(Tensor(torch.empty((0, k), dtype=torch.int32, device=t.device)),
                           Tensor(torch.empty((0, k), dtype=torch.float32, device=t.device)))
        probes = self.centroids.search(t, nprobe).indices.torch()
        indices, scores = self._launch(t, probes, k, nprobe, parts, method)
        return Matches(Tensor(indices), Tensor(scores))

    def neighbours(self, k: int = 20, nprobe: int = 8, batch: int = 8192, method: str = "grouped") -> Matches:
        """The kNN graph of the indexed rows -- the SNAPSHOT: fresh rows are neither queries nor neighbours until ``absorb`` --:
        ``Matches`` of shape (size, k), row ``i`` the ``k`` nearest OTHER indexed rows of
        original row ``i`` among the lists it probes, in ``search``'s order (-1 / -inf behind short results).  The rows are
        their own queries (exact from bf16) and go in LIST order, ``batch`` at a time: a batch then names few lists and fills
        its tiles.  Each batch is searched for ``k + 1`` -- which obeys the limits of ``search_with`` --; of every result row
        the entry that is the row itself is dropped, or the LAST entry where the row is absent (more than ``k`` equal rows
        with lower numbers come first).  ``torch`` ops on the device between the launches; nothing goes to the host.
        ``1 <= batch <= 65535``."""
        import torch
        what = "GalleryIndex.neighbours"
        if not _is_int(k):
            raise ValueError(f"{what}: k must be an integer, got {k!r}")
        if not _is_int(batch):
            raise ValueError(f"{what}: batch must be an integer, got {batch!r}")
        if batch < 1 or batch > _ffi().EMBED_LISTS_MAX_B:
            raise ValueError(f"{what}: batch = {batch}, must be in [1, {_ffi().EMBED_LISTS_MAX_B}]")
        if k < 1:
            raise ValueError(f"{what}: k = {k}, must be at least 1")
        try:
            parts = self._method_args(int(k) + 1, nprobe, 0, method, what)
        except ValueError as e:
            raise ValueError(str(e).replace(f"k = {int(k) + 1}", f"k = {k} (+ 1 for the row itself)", 1)) from None
        k, nprobe, batch = int(k), int(nprobe), int(batch)
        dev = self._rows.device
        out_idx = torch.empty((self.size, k), dtype=torch.int32, device=dev)
        out_sc = torch.empty((self.size, k), dtype=torch.float32, device=dev)
        cols = torch.arange(k, device=dev)[None, :]
        for p0 in range(0, self.size, batch):
            p1 = min(p0 + batch, self.size)
            t = self._rows[p0:p1, :self.dim].float().contiguous()
            own = self._ids[p0:p1]
            probes = self.centroids.search(t, nprobe).indices.torch()
            indices, scores = self._launch(t, probes, k + 1, nprobe, parts, method)
            is_self = indices == own[:, None]                               # at most one per row: a row is never returned twice
            at = torch.where(is_self.any(1), is_self.int().argmax(1), k)   # the column dropped: the row itself, or the last
            take = cols + (cols >= at[:, None]).long()                      # a gather of fixed shape: no synchronisation
            rows = own.long()
            out_idx[rows] = indices.gather(1, take)
            out_sc[rows] = scores.gather(1, take)
        return Matches(Tensor(out_idx), Tensor(out_sc))

    def classify(self, q, k: int = 20, nprobe: int = 8, temperature=0.07, top: int = 5, reduce: str = "sum", exclude=None) -> Votes:
        """``gallery.vote(index.search(q, k, nprobe), ...)``: the classes of the queries from their ``k`` nearest labelled rows
        among the probed lists; ``k <= 64``, and with ``exclude`` the search asks for ``k + 1`` rows as ``Gallery.classify``
        does.  Slots the lists could not fill (-1) are no candidates of the vote.  Every argument is checked first."""
        ffi = _ffi()
        what = "GalleryIndex.classify"
        g = self._gallery
        g._need_labels(what)
        inv_t, red = g._vote_args(what, temperature, top, reduce)
        if not _is_int(k):
            raise ValueError(f"{what}: k must be an integer, got {k!r}")
        extra = 0 if exclude is None else 1
        if k < 1 or k + extra > ffi.KNN_MAX_K:
            raise ValueError(f"{what}: k = {k}{' (+ 1 for the excluded row)' if extra else ''}, must be in [1, TFIMM_KNN_MAX_K = "
                             f"{ffi.KNN_MAX_K}{' - 1' if extra else ''}]")
        self._args(int(k) + extra, nprobe, 0, what)
        t = self._queries(q, what)
        up_ex = g._exclude(exclude, int(t.shape[0]), what)
        m = self.search(q, int(k) + extra, nprobe)
        return g._launch_vote(m.indices.torch(), m.scores.torch(), up_ex, inv_t, red, int(top))

    # -- the index of a gallery that grows (csrc/embed_merge.hip) ---------------------------------------------------
    def _live_args(self, k, nprobe, method, what):
        """every ``ValueError`` of ``search_live`` about ``k``, ``nprobe`` and ``method``, from both halves -- the index's
        limits are ``search_with``'s for that method, the exact search of the fresh rows has its own width limits --; returns
        (parts, the tail's arguments as ``Gallery._range_args`` gives them; None without fresh rows).  No device work."""
        try:
            parts = self._method_args(k, nprobe, 0, method, what)
        except ValueError as e:
            if "with method=" not in str(e):
                raise
            raise ValueError(str(e).replace(f"{what}: ", f"{what}: the index half refused: ", 1)) from None
        if not self.fresh:
            return parts, None
        try:
            tail = self._gallery._range_args(k, self.size, len(self._gallery), "auto", what)
        except ValueError as e:
            raise ValueError(str(e).replace(f"{what}: ", f"{what}: the exact half (the {self.fresh} fresh rows) refused: ", 1)) from None
        return parts, tail

    def _live(self, t, k, nprobe, parts, method, tail):
        """the device part of ``search_live`` for device queries ``t``, B >= 1 -> (indices, scores) torch tensors"""
        from .gallery import _merge_launch
        probes = self.centroids.search(t, nprobe).indices.torch()
        indices, scores = self._launch(t, probes, k, nprobe, parts, method)
        if tail is None:
            return indices, scores
        start, rows, ks, path = tail
        ti, ts = self._gallery._range_launch(t, ks, start, rows, path)
        return _merge_launch([(indices, scores, 0), (ti, ts, start)], k)

    def search_live(self, q, k: int = 5, nprobe: int = 8, method: str = "single") -> Matches:
        """``search`` for a gallery that has grown: per query the ``k`` best rows among the rows of the ``nprobe`` probed lists
        AND every fresh row (the rows ``size .. len(gallery)`` the snapshot does not hold) -- ``search``'s order, row
        numbers and score bits; the rule is tests/live_ref.py::search_live.  A fresh row is always found: the rows behind the
        snapshot are searched exactly (``gallery.search_range(q, k, size, len)``) and tfimm_hip_matches_merge joins the two
        results, all on the current stream, nothing goes to the host.  Without fresh rows this is ``search_with(q, k,
        nprobe, 0, method)``, launch for launch.  With ``nprobe == n_lists`` the result is ``gallery.search(q, k)``, bit for
        bit.  ``method`` is the first pass of ``search_with``; ``k`` must be acceptable to both halves -- the index's limits
        for that method and the exact search's width limits -- and the ``ValueError`` says which half refused.  The tail
        costs a scan of the fresh rows per call: ``absorb`` when they have become many."""
        import torch
        what = "GalleryIndex.search_live"
        parts, tail = self._live_args(k, nprobe, method, what)
        t = self._gallery._upload_rows(self._queries(q, what)).contiguous()
        B, k, nprobe = int(t.shape[0]), int(k), int(nprobe)
        if B == 0:
            return Matches(Tensor(torch.empty((0, k), dtype=torch.int32, device=t.device)),
                           Tensor(torch.empty((0, k), dtype=torch.float32, device=t.device)))
        indices, scores = self._live(t, k, nprobe, parts, method, tail)
        return Matches(Tensor(indices), Tensor(scores))

    def classify_live(self, q, k: int = 20, nprobe: int = 8, temperature=0.07, top: int = 5, reduce: str = "sum", exclude=None) -> Votes:
        """``classify`` over ``search_live``'s matches: enrol, then recognise -- a row added a moment ago votes.  The same
        checks, ``k <= 64`` (with ``exclude`` the search asks for ``k + 1`` rows); every argument is checked first."""
        import torch
        ffi = _ffi()
        what = "GalleryIndex.classify_live"
        g = self._gallery
        g._need_labels(what)
        inv_t, red = g._vote_args(what, temperature, top, reduce)
        if not _is_int(k):
            raise ValueError(f"{what}: k must be an integer, got {k!r}")
        extra = 0 if exclude is None else 1
        if k < 1 or k + extra > ffi.KNN_MAX_K:
            raise ValueError(f"{what}: k = {k}{' (+ 1 for the excluded row)' if extra else ''}, must be in [1, TFIMM_KNN_MAX_K = "
                             f"{ffi.KNN_MAX_K}{' - 1' if extra else ''}]")
        parts, tail = self._live_args(int(k) + extra, nprobe, "single", what)
        t = self._queries(q, what)
        up_ex = g._exclude(exclude, int(t.shape[0]), what)
        t = g._upload_rows(t).contiguous()
        if int(t.shape[0]) == 0:                                # no queries: no search, and the vote launches nothing
            return g._launch_vote(torch.empty((0, int(k) + extra), dtype=torch.int32, device=t.device),
                                  torch.empty((0, int(k) + extra), dtype=torch.float32, device=t.device), up_ex, inv_t, red, int(top))
        indices, scores = self._live(t, int(k) + extra, int(nprobe), parts, "single", tail)
        return g._launch_vote(indices, scores, up_ex, inv_t, red, int(top))

    def _assignment(self):
        """the list of every indexed row, int32 (size,), re-derived from ``ids`` and ``offsets``; no synchronisation"""
        import torch
        dev = self._ids.device
        of_pos = torch.repeat_interleave(torch.arange(self.n_lists, dtype=torch.int32, device=dev), self.counts.torch().long(),
                                         output_size=self.size)
        out = torch.empty(self.size, dtype=torch.int32, device=dev)
        out[self._ids.long()] = of_pos
        return out

    def absorb(self, assignment=None) -> int:
        """Take the fresh rows into the lists, the centroids unchanged; returns how many.  ``assignment=None`` gives each
        fresh row its best centroid (tfimm_hip_cluster_assign on that row range alone: work proportional to the fresh rows;
        the value is ``gallery.assign(index.centroids).clusters[size:]``); or pass the lists yourself, an integer array or
        ``Tensor`` of shape (fresh,) with values in [0, n_lists) -- host values are checked, a device tensor's are the
        caller's contract.  Old rows keep their list.  Afterwards the index is exactly what ``gallery.build_index(clusters=
        Clusters(centroids, old assignment ++ new assignment, ...))`` gives -- rows ascend inside a list, ``stale`` is false,
        the workspace cache is dropped.  It RE-LAYS THE WHOLE list-ordered copy: one sort of the assignment and one gather of
        all rows by ``torch`` on the device, and the build's one synchronisation -- one pass over the rows, no k-means.  The
        centroids do not follow the new rows: after much growth from another distribution recall falls, and a new
        ``build_index`` is due.  With nothing fresh it returns 0 and does nothing."""
        import torch
        what = "GalleryIndex.absorb"
        fresh = self.fresh
        new = None
        if assignment is not None:
            a = assignment.torch() if isinstance(assignment, Tensor) else assignment
            if not isinstance(a, torch.Tensor):
                a = np.asarray(a)
            kind = str(a.dtype).replace("torch.", "")
            if not kind.startswith(("int", "uint")):
                raise ValueError(f"{what}: assignment: expected integers, got {a.dtype}")
            if tuple(a.shape) != (fresh,):
                raise ValueError(f"{what}: assignment: expected shape ({fresh},) -- one list per fresh row --, got {tuple(a.shape)}")
            if fresh and not (isinstance(a, torch.Tensor) and a.is_cuda):
                lo, hi = int(a.min()), int(a.max())
                if lo < 0 or hi >= self.n_lists:
                    raise ValueError(f"{what}: assignment: lists must be in [0, n_lists = {self.n_lists}), got values in [{lo}, {hi}]")
            new = a
        if not fresh:
            return 0
        dev = self._ids.device
        if new is None:
            new = self._assign_fresh()
        elif not isinstance(new, torch.Tensor):
            new = torch.from_numpy(np.ascontiguousarray(new).astype(np.int32))
        self._lay(torch.cat([self._assignment(), new.to(dev).to(torch.int32)]))
        return fresh

    def _assign_fresh(self):
        """tfimm_hip_cluster_assign of rows ``size .. len`` against the centroids on the current stream -> int32 (fresh,)"""
        import torch
        ffi = _ffi()
        g, cen, n = self._gallery, self.centroids, self.fresh
        clusters = torch.empty(n, dtype=torch.int32, device=g._buf.device)
        scores = torch.empty(n, dtype=torch.float32, device=g._buf.device)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_cluster_assign(g._buf.data_ptr() + 2 * self.size * g.pitch, g.pitch, n, cen._buf.data_ptr(), cen.pitch,
                                                   len(cen), self.dim, clusters.data_ptr(), scores.data_ptr(), st),
                  "tfimm_hip_cluster_assign")
        return clusters


def _ffi():
    from ..engine import ffi
    return ffi


def _plan_index(gallery, n_lists, iters, init, seed, clusters):
    """every ``ValueError`` of ``Gallery.build_index`` that does not belong to ``kmeans``; returns ``n_lists`` resolved (None
    with ``clusters``).  No device work."""
    ffi = _ffi()
    what = "Gallery.build_index"
    if not len(gallery):
        raise ValueError(f"{what}: the gallery is empty")
    if clusters is not None:
        if not isinstance(clusters, Clusters) or not isinstance(clusters.centroids, Gallery):
            raise ValueError(f"{what}: clusters must be the Clusters of gallery.kmeans, got {type(clusters).__name__}")
        if n_lists is not None and n_lists != len(clusters.centroids):
            raise ValueError(f"{what}: n_lists = {n_lists!r} with clusters of {len(clusters.centroids)} centroids: leave one out")
        if clusters.centroids.dim != gallery.dim:
            raise ValueError(f"{what}: clusters of dim {clusters.centroids.dim}, this gallery holds rows of {gallery.dim}")
        if not 1 <= len(clusters.centroids) <= ffi.CLUSTER_MAX_C:
            raise ValueError(f"{what}: clusters of {len(clusters.centroids)} centroids, must be in [1, TFIMM_CLUSTER_MAX_C = "
                             f"{ffi.CLUSTER_MAX_C}]")
        if tuple(clusters.assignment.shape) != (len(gallery),):
            raise ValueError(f"{what}: clusters assign {tuple(clusters.assignment.shape)} rows, the gallery holds {len(gallery)}: "
                             f"cluster again after an add")
        return None
    if n_lists is None:
        return min(max(int(round(math.sqrt(len(gallery)))), 1), ffi.CLUSTER_MAX_C)
    return n_lists                                             # kmeans says what is wrong with it


def build_index(gallery, n_lists=None, iters=10, init=None, seed=0, clusters=None) -> GalleryIndex:
    n = _plan_index(gallery, n_lists, iters, init, seed, clusters)
    if clusters is None:
        clusters = gallery.kmeans(n, iters, init, seed)
    return GalleryIndex(gallery, clusters)
