"""
Host-side view of one device-resident forest (include/octreelib_hip.h `octl_forest`): the flat
tables behind Grid / OctreeManager / Octree.  Everything heavy (bucketing, subdivision, leaf
ordering, RANSAC, compaction) happens in HIP kernels; this module only keeps NumPy mirrors of
the small result tables and turns them into the reference's API objects lazily.
"""

import ctypes as C
from typing import Dict, List, Optional

import numpy as np

from octreelib_amd import _native as nat


class Forest:
    """mode 0 = Grid (top-level voxels of edge `edge`), mode 1 = one cube (Octree / Manager)."""

    def __init__(self, mode: int, corner, edge, ctx: Optional[nat.Context] = None):
        self.ctx = ctx if ctx is not None else nat.get_context()
        self.lib = self.ctx.lib
        self.mode = mode
        corner = np.ascontiguousarray(np.asarray(corner, dtype=np.float64).reshape(3))
        h = C.c_void_p()
        self.ctx.check(
            self.lib.octl_forest_create(self.ctx.handle, mode, nat.ptr(corner), float(edge), C.byref(h))
        )
        self.handle = h
        self.n_slots = 0
        self.slot_sizes: List[int] = []      # points ever inserted per slot
        self.slot_epoch: List[int] = []      # build epoch at which the slot's octrees were created
        self.epoch = 0                       # number of subdivide() calls so far
        self.has_scheme = False              # a K-driven scheme exists
        self._dirty = True                   # points were added since the last build
        self.info = None
        self._n_ord_pending = False
        self.n_ord = 0
        self._invalidate()
        # grid bookkeeping that must survive rebuilds: voxels each pose was inserted into and
        # the order in which voxels were first created (Grid.__octrees dict order, grid.py:56)
        self.slot_voxel_keys: List[Optional[np.ndarray]] = []
        self._edge_int = int(edge) if mode == 0 else 1
        self._cube = (tuple(np.asarray(corner, dtype=np.float64).tolist()), float(edge))
        self._creation_codes = np.empty(0, dtype=np.int64)   # packed voxel keys, creation order
        self._code_origin = None                              # voxel index the host-side codes are relative to
        self._member_next = 0                                 # first slot whose voxels have not been captured yet
        self._member_pending = []                             # (slot, voxel ids at capture time): keys not formed yet
        self._device_clouds = []                             # DeviceCloud objects whose buffers the store may read
        self._in_place = None                                # the DeviceCloud the store reads in place, if any

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.octl_forest_destroy(self.handle)
            self.handle = C.c_void_p()
            self._device_clouds = []
            self._in_place = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def reads_in_place(self, cloud) -> bool:
        return self._in_place is cloud

    def _invalidate(self):
        self._nodes = None
        self._voxels = None
        self._blocks = None
        self._order = None
        self._xyz = None
        self._perm = None
        self._slot_blocks = None
        self._counts = None
        self._internal = None
        self._pooled = None      # (pose selection, LeafPlanes) of the pooled table the device holds

    # -- points -----------------------------------------------------------------------------
    def _xf_source(self, points, transform, segment):
        """(pointer, n, flags, table, n_transforms, segment pointer, keep-alive objects) of a cloud that goes in under
        a transform (octl_forest_*_pose_xf; registration.transform_rows_np defines what is stored)."""
        from octreelib_amd.feed import DeviceCloud
        from octreelib_amd.registration import as_transform_rows

        if isinstance(points, DeviceCloud):
            src, n, flags, cloud = points.ptr, points.n, 2 | (1 if points.dtype == np.float32 else 0), points
        else:
            pts = nat.as_points_native(points)   # (f32 stays f32: widened on the device)
            src, n, flags, cloud = nat.ptr(pts), len(pts), (1 if pts.dtype == np.float32 else 0), pts
        table, seg = as_transform_rows(transform, segment, n)
        return src, n, flags, table, len(table), seg, cloud

    def add_pose(self, points, transform=None, segment=None) -> int:
        from octreelib_amd.feed import DeviceCloud

        if transform is None and segment is not None:
            raise ValueError("segment is given without transforms")
        if transform is not None:
            # moved by the ingest kernel on its way into the store; a device cloud is read in stream order, never in
            # place, and kept alive until the copy has been consumed (the next synchronising call)
            src, n, flags, table, m, seg, cloud = self._xf_source(points, transform, segment)
            slot = C.c_int32(-1)
            self.ctx.check(self.lib.octl_forest_add_pose_xf(self.handle, src, n, flags, nat.ptr(table), m, nat.ptr(seg),
                                                            C.byref(slot)))
            if flags & 2:
                self._device_clouds.append(cloud)
            self._in_place = None
            self._register_slot(n)
            return slot.value
        if isinstance(points, DeviceCloud) and points.dtype == np.float32:
            # an f32 cloud on the device: widened into the store by the library, never read in place; kept alive
            # until the copy has been consumed (the next synchronising call)
            slot = C.c_int32(-1)
            self.ctx.check(self.lib.octl_forest_add_pose_device_f32(self.handle, points.ptr, points.n, C.byref(slot)))
            self._device_clouds.append(points)
            self._in_place = None
            self._register_slot(points.n)
            return slot.value
        if isinstance(points, DeviceCloud):
            # a cloud that is (being) uploaded already: read in place when it is the first pose, copied on
            # the device otherwise; the forest keeps the object alive while it reads its buffer
            import weakref

            first = sum(self.slot_sizes) == 0 and points.n > 0   # (the library adopts iff its store is empty)
            self._device_clouds.append(points)
            slot = self.add_pose_device(points.ptr, points.n, adopt=True)
            if first:   # (only the first pose of an empty forest is read in place; later ones are copied)
                self._in_place = points
                points._readers.append(weakref.ref(self))
            else:
                self._in_place = None   # (the store grew: it is the forest's own now)
            return slot
        pts = nat.as_points_native(points)   # (f32 stays f32: the library widens it on the device)
        slot = C.c_int32(-1)
        fn = self.lib.octl_forest_add_pose_f32 if pts.dtype == np.float32 else self.lib.octl_forest_add_pose
        self.ctx.check(fn(self.handle, nat.ptr(pts), len(pts), C.byref(slot)))
        self._in_place = None
        self._register_slot(len(pts))
        return slot.value

    def add_pose_device(self, dptr, n: int, adopt: bool = False) -> int:
        """A cloud that is in device memory already.  adopt=True: an empty forest reads the caller's buffer in
        place (no copy; the buffer must stay alive and unchanged until the forest is cleared or closed)."""
        slot = C.c_int32(-1)
        fn = self.lib.octl_forest_add_pose_adopt if adopt else self.lib.octl_forest_add_pose_device
        self.ctx.check(fn(self.handle, dptr, int(n), C.byref(slot)))
        self._register_slot(int(n))
        return slot.value

    def add_pose_routed(self, n: int) -> int:
        slot = C.c_int32(-1)
        self.ctx.check(self.lib.octl_forest_add_pose_routed(self.handle, C.byref(slot)))
        self._register_slot(int(n))
        return slot.value

    def _register_slot(self, n: int):
        self.n_slots += 1
        self.slot_sizes.append(n)
        self.slot_epoch.append(self.epoch)
        self.slot_voxel_keys.append(None)
        self._dirty = True
        self._invalidate()

    def extend_pose(self, slot: int, points, transform=None, segment=None):
        from octreelib_amd.feed import DeviceCloud

        if transform is None and segment is not None:
            raise ValueError("segment is given without transforms")
        if transform is not None:
            src, n_new, flags, table, m, seg, cloud = self._xf_source(points, transform, segment)
            self.ctx.check(self.lib.octl_forest_extend_pose_xf(self.handle, slot, src, n_new, flags, nat.ptr(table), m,
                                                               nat.ptr(seg)))
            if flags & 2:
                self._device_clouds.append(cloud)
        elif isinstance(points, DeviceCloud):
            # appended device-to-device behind the pose's points (the library orders the copy behind the upload)
            fn = (self.lib.octl_forest_extend_pose_device_f32 if points.dtype == np.float32
                  else self.lib.octl_forest_extend_pose_device)
            self.ctx.check(fn(self.handle, slot, points.ptr, points.n))
            self._device_clouds.append(points)   # (alive until the copy has been consumed by the next build)
            n_new = points.n
        else:
            pts = nat.as_points_native(points)
            fn = self.lib.octl_forest_extend_pose_f32 if pts.dtype == np.float32 else self.lib.octl_forest_extend_pose
            self.ctx.check(fn(self.handle, slot, nat.ptr(pts), len(pts)))
            n_new = len(pts)
        self._in_place = None
        self.slot_sizes[slot] += n_new
        self._dirty = True
        self._invalidate()

    # -- build ------------------------------------------------------------------------------
    def build(self, K: int, scheme_slots=None, keep_scheme=False, max_depth=0):
        self._resolve_membership()   # (captured voxel ids refer to the voxel table this build may renumber)
        mask = None
        if scheme_slots is not None and not keep_scheme:
            mask = np.zeros(self.n_slots, dtype=np.uint8)
            mask[list(scheme_slots)] = 1
        info = nat.BuildInfo()
        try:
            self.ctx.check(
                self.lib.octl_forest_build(
                    self.handle, int(K), nat.ptr(mask), self.n_slots if mask is not None else 0,
                    1 if keep_scheme else 0, int(max_depth), C.byref(info),
                )
            )
        except (RecursionError, nat.DomainError, MemoryError, RuntimeError):
            # the library dropped the scheme (include/octreelib_hip.h): the next query rebuilds the
            # top-level voxels; the reference leaves a half-subdivided tree behind in these cases
            self.has_scheme = False
            self._dirty = True
            self.info = None
            self._invalidate()
            raise
        self.info = info
        self.n_ord = int(info.n_points)
        self._dirty = False
        self._invalidate()
        if not keep_scheme:
            self.epoch += 1
            self.has_scheme = True
        self._update_membership()

    def subdivide(self, K: int, scheme_slots=None, max_depth=0):
        self.build(K, scheme_slots, False, max_depth)

    def subdivide_planar(self, rule, scheme_slots=None, max_depth=0):
        """Subdivision by `rule` = (K, max_variance, min_points, ddof) of criteria.try_planar_threshold: count > K
        OR NotPlanar, decided inside the level loop on the device (octl_forest_build_planar)."""
        k, max_variance, min_points, ddof = rule
        self._resolve_membership()
        mask = None
        if scheme_slots is not None:
            mask = np.zeros(self.n_slots, dtype=np.uint8)
            mask[list(scheme_slots)] = 1
        info = nat.BuildInfo()
        try:
            self.ctx.check(
                self.lib.octl_forest_build_planar(
                    self.handle, int(k), float(max_variance), int(min_points), int(ddof), nat.ptr(mask),
                    self.n_slots if mask is not None else 0, int(max_depth), C.byref(info),
                )
            )
        except (RecursionError, nat.DomainError, MemoryError, RuntimeError):
            self.has_scheme = False   # (the library dropped the scheme: see build)
            self._dirty = True
            self.info = None
            self._invalidate()
            raise
        self.info = info
        self.n_ord = int(info.n_points)
        self._dirty = False
        self._invalidate()
        self.epoch += 1
        self.has_scheme = True
        self._update_membership()

    def split_stats(self):
        """(n_scheme u32, lambda_min f64) per scheme node: what the split decisions of the last planar subdivide
        saw (octl_forest_get_split_stats); NaN where no statistic was evaluated."""
        self.ensure_built()
        n = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_get_split_stats(self.handle, 0, None, None, C.byref(n)))
        cnt = np.empty(n.value, dtype=np.uint32)
        lam = np.empty(n.value, dtype=np.float64)
        if n.value:
            self.ctx.check(self.lib.octl_forest_get_split_stats(self.handle, n.value, nat.ptr(cnt), nat.ptr(lam),
                                                                C.byref(n)))
        return cnt, lam

    def subdivide_callable(self, criteria, scheme_slots=None, max_depth=63):
        """Subdivision driven by arbitrary host callables (octree.py:26: a node splits when
        any(criterion(points))).  A Python callable cannot run inside a kernel: the host evaluates
        the predicates level by level on the points of the scheme octree's nodes (the union of the
        selected poses, octree_manager.py:53-61) and installs the resulting scheme; every placement
        (bucketing, partition into leaves, ordering) still happens on the device.  Cost: one
        device re-placement per tree level - meant for API completeness, not for speed.
        The order of the rows handed to a criterion is pose-major / insertion order (the
        reference's order is an artefact of an unstable argsort)."""
        self.ensure_built()
        self._resolve_membership()
        scheme = set(range(self.n_slots)) if scheme_slots is None else set(scheme_slots)
        # epochs of nodes that stay internal are inherited (cached-leaf order is history dependent)
        prev = {}
        if self.has_scheme:
            nd = self.nodes
            path = _node_paths(nd)
            vox = self.voxels
            for i in np.nonzero(nd["first_child"] >= 0)[0]:
                prev[(tuple(vox[nd["voxel"][i]]), path[i])] = int(nd["epoch"][i])
        new_epoch = self.epoch + 1
        V = len(self.voxels)
        vox_keys = [tuple(v) for v in self.voxels.tolist()]
        fc = [-1] * V
        ep = [0] * V
        node_vox = list(range(V))
        node_path = [()] * V
        frontier = list(range(V))
        empty = np.empty((0, 3), dtype=float)
        depth = 0
        while True:
            fca = np.ascontiguousarray(np.array(fc, dtype=np.int32))
            epa = np.ascontiguousarray(np.array(ep, dtype=np.int32))
            self.ctx.check(self.lib.octl_forest_set_scheme(self.handle, nat.ptr(fca), nat.ptr(epa), len(fca), new_epoch))
            info = nat.BuildInfo()
            self.ctx.check(self.lib.octl_forest_build(self.handle, 0, None, 0, 1, 0, C.byref(info)))
            self.info = info
            self.n_ord = int(info.n_points)
            self._dirty = False
            self._invalidate()
            assert np.array_equal(self.nodes["first_child"], fca), "device and host node numbering differ"
            if not frontier:
                break
            blk = self.blocks
            xyz = self.xyz
            by_node = {}
            for n, s_, st, sz in zip(blk["node"].tolist(), blk["slot"].tolist(), blk["start"].tolist(), blk["size"].tolist()):
                if s_ in scheme:
                    by_node.setdefault(n, []).append((st, sz))
            to_split = []
            for n in frontier:
                parts = by_node.get(n)
                pts = np.vstack([xyz[a : a + b] for a, b in parts]) if parts else empty
                if any([c(pts) for c in criteria]):
                    to_split.append(n)
            if not to_split:
                break
            depth += 1
            if depth > max_depth:
                raise RecursionError(f"maximum depth {max_depth} exceeded")
            frontier = []
            for n in sorted(to_split):
                fc[n] = len(fc)
                key = (vox_keys[node_vox[n]], node_path[n])
                ep[n] = prev.get(key, new_epoch)
                for j in range(8):
                    frontier.append(len(fc))
                    fc.append(-1)
                    ep.append(0)
                    node_vox.append(node_vox[n])
                    node_path.append(node_path[n] + (j,))
        self.epoch = new_epoch
        self.has_scheme = True
        self._update_membership()

    def adopt_scheme(self, other: "Forest"):
        """Make this forest's scheme the scheme of `other` (OctreeNode.subdivide_as, octree.py:34-53:
        split wherever `other` is split).  Both forests must cover the same voxels.  Nodes that
        are already internal here keep their epoch (the cached-leaf order is history dependent),
        newly split ones get a new epoch; where this forest is finer than `other` the subtree is
        merged (upstream's merge branch is defective, SURVEY 8 a8 - outside the parity domain)."""
        self.ensure_built()
        other.ensure_built()
        self._resolve_membership()
        if self.mode != other.mode or self._cube != other._cube or not np.array_equal(self.voxels, other.voxels):
            raise ValueError("subdivide_as needs two octrees over the same cube")
        ond = other.nodes
        ofc = np.ascontiguousarray(ond["first_child"], dtype=np.int32)
        prev = {}
        if self.has_scheme:
            nd = self.nodes
            path = _node_paths(nd)
            for i in np.nonzero(nd["first_child"] >= 0)[0]:
                prev[(int(nd["voxel"][i]), path[i])] = int(nd["epoch"][i])
        new_epoch = self.epoch + 1
        opath = _node_paths(ond)
        ep = np.zeros(len(ofc), dtype=np.int32)
        for i in np.nonzero(ofc >= 0)[0]:
            ep[i] = prev.get((int(ond["voxel"][i]), opath[i]), new_epoch)
        self.ctx.check(self.lib.octl_forest_set_scheme(self.handle, nat.ptr(ofc), nat.ptr(ep), len(ofc), new_epoch))
        info = nat.BuildInfo()
        self.ctx.check(self.lib.octl_forest_build(self.handle, 0, None, 0, 1, 0, C.byref(info)))
        self.info = info
        self.n_ord = int(info.n_points)
        self._dirty = False
        self._invalidate()
        self.epoch = new_epoch
        self.has_scheme = True
        self._update_membership()

    def ensure_built(self):
        """Bring the device structure up to date after insertions: a new pose inherits the
        current scheme (octree_manager.py:161-171); before any subdivide the scheme is just
        the top-level voxels."""
        if not self._dirty and self.info is not None:
            return
        if self.has_scheme:
            self.build(0, None, keep_scheme=True)
        else:
            self._resolve_membership()
            # K < 0: never split.  Not a subdivide call: the epoch does not advance.
            info = nat.BuildInfo()
            self.ctx.check(self.lib.octl_forest_build(self.handle, -1, None, 0, 0, 0, C.byref(info)))
            self.info = info
            self.n_ord = int(info.n_points)
            self._dirty = False
            self._invalidate()
            self.epoch += 1  # mirrors the library's counter of non-keep builds
            self._update_membership()

    def _update_membership(self):
        """Capture, for slots seen for the first time, the voxels they were inserted into
        (Grid.__pose_voxel_coordinates, grid.py:53,108) - as voxel ids of the table of THIS build; the keys and
        the voxel creation order are formed when someone asks or before the table can change
        (_resolve_membership): a scan that is built, fitted and dropped never pays for them."""
        for s in range(self._member_next, self.n_slots):
            n = C.c_int64(0)
            self.ctx.check(self.lib.octl_forest_get_slot_voxels(self.handle, s, 0, None, C.byref(n)))
            vids = np.empty(n.value, dtype=np.int32)
            if n.value:
                self.ctx.check(
                    self.lib.octl_forest_get_slot_voxels(self.handle, s, n.value, nat.ptr(vids), C.byref(n))
                )
            self._member_pending.append((s, vids))
        self._member_next = self.n_slots

    def _fetch_voxels(self) -> np.ndarray:
        """The library's voxel table as it stands (no build is triggered)."""
        n = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_get_voxels(self.handle, 0, None, C.byref(n)))
        v = np.empty((n.value, 3), dtype=np.int64)
        self.ctx.check(self.lib.octl_forest_get_voxels(self.handle, n.value, nat.ptr(v), C.byref(n)))
        return v

    def _resolve_membership(self):
        if not self._member_pending:
            return
        vox = self._voxels if self._voxels is not None else self._fetch_voxels()
        for s, vids in self._member_pending:
            keys = vox[vids]
            self.slot_voxel_keys[s] = keys
            # voxels seen for the first time, in this pose's (lexicographic = np.unique) order
            codes = self._voxel_codes(keys)
            fresh = codes[~np.isin(codes, self._creation_codes)]
            if len(fresh):
                self._creation_codes = np.concatenate((self._creation_codes, fresh))
        self._member_pending = []

    def _voxel_codes(self, keys: np.ndarray) -> np.ndarray:
        """(m,3) int64 voxel corners -> one int64 per voxel (bijective: |index| < 2^20 per axis,
        include/octreelib_hip.h)."""
        q = np.asarray(keys, dtype=np.int64).reshape(-1, 3) // self._edge_int
        if self._code_origin is None:
            if len(q) == 0:
                return np.empty(0, dtype=np.int64)
            self._code_origin = q.min(axis=0)   # codes are relative to where the scene started (any int64 index)
        q = q - self._code_origin + (1 << 20)
        if len(q) and (q.min() < 0 or q.max() >= (1 << 21)):
            raise nat.DomainError("the scene has moved more than 2^20 voxels away from where it started")
        return (q[:, 0] << 42) | (q[:, 1] << 21) | q[:, 2]

    def creation_ranks(self, keys: np.ndarray) -> np.ndarray:
        """Position of every voxel of `keys` in the order voxels were first created
        (the dict order of Grid.__octrees, grid.py:56,100-109)."""
        self._resolve_membership()
        order = np.argsort(self._creation_codes, kind="stable")
        pos = np.searchsorted(self._creation_codes[order], self._voxel_codes(keys))
        return order[pos].astype(np.int64)

    # -- tables -----------------------------------------------------------------------------
    @property
    def nodes(self):
        if self._nodes is None:
            self.ensure_built()
            n = C.c_int64(0)
            self.ctx.check(
                self.lib.octl_forest_get_nodes(self.handle, 0, None, None, None, None, None, None, None, C.byref(n))
            )
            n = n.value
            t = {
                "voxel": np.empty(n, dtype=np.int32),
                "depth": np.empty(n, dtype=np.int32),
                "parent": np.empty(n, dtype=np.int32),
                "first_child": np.empty(n, dtype=np.int32),
                "corner": np.empty((n, 3), dtype=np.float64),
                "edge": np.empty(n, dtype=np.float64),
                "epoch": np.empty(n, dtype=np.int32),
            }
            m = C.c_int64(0)
            self.ctx.check(
                self.lib.octl_forest_get_nodes(
                    self.handle, n, nat.ptr(t["voxel"]), nat.ptr(t["depth"]), nat.ptr(t["parent"]),
                    nat.ptr(t["first_child"]), nat.ptr(t["corner"]), nat.ptr(t["edge"]),
                    nat.ptr(t["epoch"]), C.byref(m),
                )
            )
            self._nodes = t
        return self._nodes

    @property
    def voxels(self) -> np.ndarray:
        """(V,3) int64 voxel coordinates (= corners), lexicographic order."""
        if self._voxels is None:
            self.ensure_built()
            n = C.c_int64(0)
            self.ctx.check(self.lib.octl_forest_get_voxels(self.handle, 0, None, C.byref(n)))
            v = np.empty((n.value, 3), dtype=np.int64)
            self.ctx.check(self.lib.octl_forest_get_voxels(self.handle, n.value, nat.ptr(v), C.byref(n)))
            self._voxels = v
        return self._voxels

    @property
    def blocks(self):
        if self._blocks is None:
            self.ensure_built()
            n = C.c_int64(0)
            self.ctx.check(self.lib.octl_forest_get_blocks(self.handle, 0, None, None, None, None, C.byref(n)))
            n = n.value
            b = {
                "node": np.empty(n, dtype=np.int32),
                "slot": np.empty(n, dtype=np.int32),
                "start": np.empty(n, dtype=np.int64),
                "size": np.empty(n, dtype=np.int32),
            }
            m = C.c_int64(0)
            self.ctx.check(
                self.lib.octl_forest_get_blocks(
                    self.handle, n, nat.ptr(b["node"]), nat.ptr(b["slot"]), nat.ptr(b["start"]),
                    nat.ptr(b["size"]), C.byref(m),
                )
            )
            self._blocks = b
        return self._blocks

    @property
    def order(self) -> np.ndarray:
        """All non-empty (leaf, pose) blocks in the reference's listing order (slot major,
        voxel lexicographic, cached-leaf order) - computed on the device."""
        if self._order is None:
            self.ensure_built()
            nb = len(self.blocks["node"])
            e0 = np.ascontiguousarray(np.asarray(self.slot_epoch, dtype=np.int32))
            out = np.empty(nb, dtype=np.int32)
            n = C.c_int64(0)
            self.ctx.check(
                self.lib.octl_forest_reference_order(
                    self.handle, nat.ptr(e0) if self.n_slots else None, self.n_slots, nb,
                    nat.ptr(out), C.byref(n),
                )
            )
            self._order = out
        return self._order

    def slot_blocks(self, slot: int) -> np.ndarray:
        """Block ids of a slot in the reference's order (= its non-empty leaves)."""
        if self._slot_blocks is None:
            order = self.order
            slots = self.blocks["slot"][order]
            # order is slot-major: split at the slot boundaries
            bounds = np.searchsorted(slots, np.arange(self.n_slots + 1))
            self._slot_blocks = [order[bounds[s] : bounds[s + 1]] for s in range(self.n_slots)]
        return self._slot_blocks[slot]

    @property
    def xyz(self) -> np.ndarray:
        """Leaf-ordered coordinates (n,3) f64 (host copy, fetched on first use)."""
        if self._xyz is None:
            self.ensure_built()
            n = self.n_ord
            a = np.empty((n, 3), dtype=np.float64)
            if n:
                self.ctx.check(self.lib.octl_forest_get_points(self.handle, 0, n, nat.ptr(a)))
            self._xyz = a
        return self._xyz

    def gather_blocks(self, block_ids) -> np.ndarray:
        """Rows of the given blocks, concatenated in the given order: ONE device gather and one download
        (octl_forest_gather_blocks) - what the reference's get_points loops concatenate leaf by leaf
        (grid.py:234-242, octree_manager.py:121-130, octree.py:55-65).  A host copy of the whole ordered cloud that
        is there already is sliced instead."""
        ids = np.ascontiguousarray(block_ids, dtype=np.int32)
        if len(ids) == 0:
            return np.empty((0, 3), dtype=float)
        blk = self.blocks
        if self._xyz is not None:
            starts = blk["start"][ids].astype(np.int64)
            sizes = blk["size"][ids].astype(np.int64)
            offs = np.cumsum(sizes) - sizes
            idx = np.repeat(starts - offs, sizes) + np.arange(int(sizes.sum()), dtype=np.int64)
            return self._xyz[idx]
        self.ensure_built()
        n = int(blk["size"][ids].sum())
        out = np.empty((n, 3), dtype=np.float64)
        got = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_gather_blocks(self.handle, nat.ptr(ids), len(ids), n, nat.ptr(out),
                                                          C.byref(got)))
        if got.value != n:
            raise RuntimeError(f"gather_blocks: {got.value} rows on the device, {n} in the host's block table")
        return out

    def leaf_stats(self, block_ids, eigen: bool = True):
        """Point count, mean, population covariance and (eigen=True) its eigen-decomposition of every given block,
        computed on the device in one call (octl_forest_leaf_stats): a LeafStatistics whose row i describes
        block_ids[i].  With eigen=False its eigenvalues / eigenvectors are None."""
        from octreelib_amd.leaf_stats import LeafStatistics, cov6_to_full

        ids = np.ascontiguousarray(block_ids, dtype=np.int32).reshape(-1)
        self.ensure_built()
        n = len(ids)
        count = np.empty(n, dtype=np.int64)
        mean = np.empty((n, 3), dtype=np.float64)
        cov = np.empty((n, 6), dtype=np.float64)
        w = np.empty((n, 3), dtype=np.float64) if eigen else None
        v = np.empty((n, 3, 3), dtype=np.float64) if eigen else None
        self.ctx.check(self.lib.octl_forest_leaf_stats(self.handle, nat.ptr(ids), n, nat.ptr(count), nat.ptr(mean),
                                                       nat.ptr(cov), nat.ptr(w), nat.ptr(v)))
        return LeafStatistics(count, mean, cov6_to_full(cov), w, v)

    # -- queries (octreelib_amd/query.py is the host definition of each) -----------------------------------------
    def locate(self, points) -> np.ndarray:
        """int32 node id of the scheme leaf every query point falls into, -1 where there is none
        (octl_forest_locate: one kernel, read-only)."""
        from octreelib_amd.query import _as_queries

        pts = _as_queries(points)
        self.ensure_built()
        out = np.empty(len(pts), dtype=np.int32)
        if len(pts):
            self.ctx.check(self.lib.octl_forest_locate(self.handle, nat.ptr(pts), len(pts), nat.ptr(out)))
        return out

    def locate_device(self, xyz_dptr, n: int, node_dptr):
        """locate for points that are in device memory already, answers left there (pointers from octl_dev_alloc);
        enqueued on the context's stream, the host does not wait."""
        self.ensure_built()
        self.ctx.check(self.lib.octl_forest_locate_device(self.handle, xyz_dptr, int(n), node_dptr))

    def leaf_planes(self, slots=None):
        """One plane per leaf over the poses of `slots` (None: all), all their points pooled
        (octl_forest_pooled_leaf_stats): a LeafPlanes in ascending node id.  The device keeps the table for
        point_to_plane; the same selection on an unchanged forest is answered from the copy made here."""
        from octreelib_amd.leaf_stats import cov6_to_full
        from octreelib_amd.query import LeafPlanes

        self.ensure_built()
        key = None if slots is None else tuple(sorted(set(int(s) for s in slots)))
        if self._pooled is not None and self._pooled[0] == key:
            return self._pooled[1]
        sel = None
        if key is not None and self.n_slots > 0:
            sel = np.zeros(self.n_slots, dtype=np.uint8)
            sel[list(key)] = 1
        n_sel = self.n_slots if sel is not None else 0
        n = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_pooled_leaf_stats(self.handle, nat.ptr(sel), n_sel, 0, None, None, None,
                                                              None, None, None, C.byref(n)))
        m = n.value
        node = np.empty(m, dtype=np.int32)
        count = np.empty(m, dtype=np.int64)
        mean = np.empty((m, 3), dtype=np.float64)
        cov = np.empty((m, 6), dtype=np.float64)
        w = np.empty((m, 3), dtype=np.float64)
        v = np.empty((m, 3, 3), dtype=np.float64)
        if m:
            self.ctx.check(self.lib.octl_forest_pooled_leaf_stats(
                self.handle, nat.ptr(sel), n_sel, m, nat.ptr(node), nat.ptr(count), nat.ptr(mean), nat.ptr(cov),
                nat.ptr(w), nat.ptr(v), C.byref(n)))
        planes = LeafPlanes(count, mean, cov6_to_full(cov), w, v, node)
        self._pooled = (key, planes)
        return planes

    def point_to_plane(self, points, slots=None, min_points: int = 8, max_variance=None):
        """Leaf, plane row and signed distance of every query point (octl_forest_point_to_plane: one fused kernel);
        the pooled table is recomputed only when the device one is stale or was made for another selection."""
        from octreelib_amd.query import PointToPlane, _as_queries

        pts = _as_queries(points)
        planes = self.leaf_planes(slots)
        n = len(pts)
        node = np.empty(n, dtype=np.int32)
        row = np.empty(n, dtype=np.int32)
        dist = np.empty(n, dtype=np.float64)
        if n:
            mv = -1.0 if max_variance is None else float(max_variance)
            self.ctx.check(self.lib.octl_forest_point_to_plane(self.handle, nat.ptr(pts), n, int(min_points), mv,
                                                               nat.ptr(node), nat.ptr(row), nat.ptr(dist)))
        return PointToPlane(node, row, dist, planes)

    def point_to_plane_device(self, xyz_dptr, n: int, node_dptr, row_dptr, dist_dptr, min_points: int = 8,
                              max_variance=None):
        """point_to_plane against the pooled table the device holds (leaf_planes first), device pointers in and
        out; the host does not wait."""
        mv = -1.0 if max_variance is None else float(max_variance)
        self.ctx.check(self.lib.octl_forest_point_to_plane_device(self.handle, xyz_dptr, int(n), int(min_points), mv,
                                                                  node_dptr, row_dptr, dist_dptr))

    def nearest(self, points, k: int = 1, max_distance=None, slots=None):
        """The k stored points of the poses of `slots` (None: all) nearest to every query point within max_distance
        (octl_forest_nearest: one kernel once the block index of the selection exists): (slot (n, k) int32, index
        (n, k) int64, distance2 (n, k) float64, count (n,) int32) as query.nearest_np defines them, the pose given by
        its slot."""
        from octreelib_amd.query import _as_queries, check_nearest_args

        k, r = check_nearest_args(k, max_distance)
        pts = _as_queries(points)
        self.ensure_built()
        sel, n_sel, _ = self._adjust_selection(slots)
        n = len(pts)
        slot = np.full((n, k), -1, dtype=np.int32)
        index = np.full((n, k), -1, dtype=np.int64)
        d2 = np.full((n, k), np.inf, dtype=np.float64)
        count = np.zeros(n, dtype=np.int32)
        # (n = 0 still goes to the library: what it refuses whatever the queries is refused for an empty scan too)
        self.ctx.check(self.lib.octl_forest_nearest(self.handle, nat.ptr(pts), n, k, r, nat.ptr(sel), n_sel,
                                                    nat.ptr(slot), nat.ptr(index), nat.ptr(d2), nat.ptr(count)))
        return slot, index, d2, count

    def nearest_device(self, xyz_dptr, n: int, k: int, max_distance, slot_dptr, index_dptr, d2_dptr, count_dptr,
                       slots=None):
        """nearest for points that are in device memory already, the (n, k) / (n,) answers left there (pointers from
        octl_dev_alloc); enqueued on the context's stream, the host does not wait."""
        from octreelib_amd.query import check_nearest_args

        k, r = check_nearest_args(k, max_distance)
        self.ensure_built()
        sel, n_sel, _ = self._adjust_selection(slots)
        self.ctx.check(self.lib.octl_forest_nearest_device(self.handle, xyz_dptr, int(n), k, r, nat.ptr(sel), n_sel,
                                                           slot_dptr, index_dptr, d2_dptr, count_dptr))

    def neighbours(self, points, k, max_distance, slots, pose_of_slot):
        """nearest as a query.Neighbours: pose_of_slot maps the slot column to pose numbers (None: slots are the
        pose numbers)."""
        from octreelib_amd.query import Neighbours

        slot, index, d2, count = self.nearest(points, k, max_distance, slots)
        if pose_of_slot is not None and slot.size:
            names = np.asarray(list(pose_of_slot) + [-1], dtype=np.int32)   # (-1 pads index the last entry)
            slot = names[slot]
        return Neighbours(slot, index, d2, count)

    def radius_count(self, points, radius, max_count=None, slots=None) -> np.ndarray:
        """How many stored points of the poses of `slots` (None: all) lie within `radius` of every query point, capped
        at max_count (None: uncapped): (n,) int32 as query.radius_count_np defines it (octl_forest_radius_count: one
        kernel once the block index of the selection exists).  points: a host array, or a feed.DeviceCloud of f64
        points, which is read where it lies."""
        from octreelib_amd.feed import DeviceCloud
        from octreelib_amd.query import _as_queries, check_radius_args

        r, max_count, _ = check_radius_args(radius, max_count)
        cap = 0 if max_count is None else max_count
        if isinstance(points, DeviceCloud):
            if np.dtype(points.dtype) != np.float64:
                raise ValueError("radius_count: a DeviceCloud of float64 points is needed (f32 queries are not "
                                 "supported)")
            points.wait()
            n = len(points)
            count = np.zeros(n, dtype=np.int32)
            lib, h = self.lib, self.ctx.handle
            out = C.c_void_p()
            self.ctx.check(lib.octl_dev_alloc(h, max(4 * n, 8), C.byref(out)))
            try:
                self.radius_count_device(points.ptr, n, r, out, max_count, slots)
                if n:
                    self.ctx.check(lib.octl_dev_download(h, nat.ptr(count), out, count.nbytes))
            finally:
                lib.octl_dev_free(h, out)
            return count
        pts = _as_queries(points)
        self.ensure_built()
        sel, n_sel, _ = self._adjust_selection(slots)
        n = len(pts)
        count = np.zeros(n, dtype=np.int32)
        # (n = 0 still goes to the library: what it refuses whatever the queries is refused for an empty scan too)
        self.ctx.check(self.lib.octl_forest_radius_count(self.handle, nat.ptr(pts), n, r, cap, nat.ptr(sel), n_sel,
                                                         nat.ptr(count)))
        return count

    def radius_count_device(self, xyz_dptr, n: int, radius, count_dptr, max_count=None, slots=None):
        """radius_count for points that are in device memory already, the (n,) int32 answer left there (pointers from
        octl_dev_alloc); enqueued on the context's stream, the host does not wait."""
        from octreelib_amd.query import check_radius_args

        r, max_count, _ = check_radius_args(radius, max_count)
        self.ensure_built()
        sel, n_sel, _ = self._adjust_selection(slots)
        self.ctx.check(self.lib.octl_forest_radius_count_device(self.handle, xyz_dptr, int(n), r,
                                                                0 if max_count is None else max_count, nat.ptr(sel),
                                                                n_sel, count_dptr))

    def remove_sparse(self, radius, min_neighbours, slots=None, among=None) -> int:
        """Radius outlier removal: every point of the poses of `slots` (None: all) with fewer than min_neighbours other
        points of the poses of `among` (None: all) within `radius` leaves the map (octl_forest_remove_sparse: one
        kernel, one compaction that also applies a pending RANSAC mask; query.sparse_keep_np is the rule); the scheme
        stays.  Returns the number of points removed."""
        from octreelib_amd.query import _required, check_radius_args

        r, _, m = check_radius_args(radius, None, _required(min_neighbours), what="remove_sparse")
        self.ensure_built()
        before = self.n_ord
        sel, n_sel, _ = self._adjust_selection(slots)
        asel, n_asel, _ = self._adjust_selection(among)
        n = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_remove_sparse(self.handle, r, m, nat.ptr(sel), n_sel, nat.ptr(asel), n_asel,
                                                          C.byref(n)))
        self.n_ord = n.value
        self._invalidate()
        return before - n.value

    def neighbourhood_stats(self, points, radius, slots=None, eigen: bool = True):
        """Count, mean, population covariance and (eigen=True) its eigen-decomposition of the stored points of the poses
        of `slots` (None: all) within `radius` of every query point: a LeafStatistics with one row per query, as
        neighbourhood.neighbourhood_statistics_np defines it (octl_forest_neighbourhood_stats: one kernel once the block
        index of the selection exists).  points: a host array, or a feed.DeviceCloud of f64 points, which is read where
        it lies."""
        from octreelib_amd.feed import DeviceCloud
        from octreelib_amd.leaf_stats import LeafStatistics, cov6_to_full
        from octreelib_amd.query import _as_queries, check_radius_args

        r, _, _ = check_radius_args(radius, what="neighbourhood_statistics")
        device = isinstance(points, DeviceCloud)
        if device:
            if np.dtype(points.dtype) != np.float64:
                raise ValueError("neighbourhood_statistics: a DeviceCloud of float64 points is needed (f32 queries "
                                 "are not supported)")
            points.wait()
            n = len(points)
        else:
            pts = _as_queries(points)
            n = len(pts)
        count = np.zeros(n, dtype=np.int64)
        mean = np.empty((n, 3), dtype=np.float64)
        cov = np.empty((n, 6), dtype=np.float64)
        w = np.empty((n, 3), dtype=np.float64) if eigen else None
        v = np.empty((n, 3, 3), dtype=np.float64) if eigen else None
        outs = [a for a in (count, mean, cov, w, v) if a is not None]
        if device:
            lib, h = self.lib, self.ctx.handle
            bufs = [C.c_void_p() for _ in outs]
            try:
                for b, a in zip(bufs, outs):
                    self.ctx.check(lib.octl_dev_alloc(h, max(a.nbytes, 8), C.byref(b)))
                self.neighbourhood_stats_device(points.ptr, n, r, *bufs[:3], *(bufs[3:] if eigen else (None, None)),
                                                slots=slots)
                for b, a in zip(bufs, outs):
                    if n:
                        self.ctx.check(lib.octl_dev_download(h, nat.ptr(a), b, a.nbytes))
            finally:
                for b in bufs:
                    if b.value:
                        lib.octl_dev_free(h, b)
        else:
            self.ensure_built()
            sel, n_sel, _ = self._adjust_selection(slots)
            # (n = 0 still goes to the library: what it refuses whatever the queries is refused for an empty scan too)
            self.ctx.check(self.lib.octl_forest_neighbourhood_stats(self.handle, nat.ptr(pts), n, r, nat.ptr(sel),
                                                                    n_sel, nat.ptr(count), nat.ptr(mean), nat.ptr(cov),
                                                                    nat.ptr(w), nat.ptr(v)))
        return LeafStatistics(count, mean, cov6_to_full(cov), w, v)

    def neighbourhood_stats_device(self, xyz_dptr, n: int, radius, count_dptr, mean_dptr, cov_dptr, eigval_dptr=None,
                                   eigvec_dptr=None, slots=None):
        """neighbourhood_stats for points that are in device memory already, the rows - count (n,) int64, mean (n, 3),
        cov (n, 6), eigval (n, 3), eigvec (n, 3, 3) float64; the last two None: no decomposition - left there (pointers
        from octl_dev_alloc); enqueued on the context's stream, the host does not wait."""
        from octreelib_amd.query import check_radius_args

        r, _, _ = check_radius_args(radius, what="neighbourhood_statistics")
        self.ensure_built()
        sel, n_sel, _ = self._adjust_selection(slots)
        self.ctx.check(self.lib.octl_forest_neighbourhood_stats_device(self.handle, xyz_dptr, int(n), r, nat.ptr(sel),
                                                                       n_sel, count_dptr, mean_dptr, cov_dptr,
                                                                       eigval_dptr, eigvec_dptr))

    def point_stats(self, radius, slots=None, among=None, eigen: bool = True, pose_of_slot=None):
        """The self-query: one row of neighbourhood_stats for every alive stored point of the poses of `slots` (None:
        all) over the stored points of the poses of `among` (None: all), the point itself included when its pose is
        counted: a neighbourhood.PointStatistics in ascending (slot, index) (octl_forest_point_stats: one kernel once
        the block index of `among` exists; nothing of the map changes).  pose_of_slot maps slots to pose numbers (None:
        slots are the pose numbers)."""
        from octreelib_amd.leaf_stats import cov6_to_full
        from octreelib_amd.neighbourhood import PointStatistics
        from octreelib_amd.query import check_radius_args

        r, _, _ = check_radius_args(radius, what="point_statistics")
        self.ensure_built()
        sel, n_sel, chosen = self._adjust_selection(slots)
        asel, n_asel, _ = self._adjust_selection(among)
        cap = min(int(self.n_ord), int(sum(self.slot_sizes[s] for s in chosen)))
        rows = C.c_int64(0)
        for _ in range(2):
            slot = np.empty(cap, dtype=np.int32)
            index = np.empty(cap, dtype=np.int32)
            count = np.empty(cap, dtype=np.int64)
            mean = np.empty((cap, 3), dtype=np.float64)
            cov = np.empty((cap, 6), dtype=np.float64)
            w = np.empty((cap, 3), dtype=np.float64) if eigen else None
            v = np.empty((cap, 3, 3), dtype=np.float64) if eigen else None
            self.ctx.check(self.lib.octl_forest_point_stats(self.handle, r, nat.ptr(sel), n_sel, nat.ptr(asel), n_asel,
                                                            cap, C.byref(rows), nat.ptr(slot), nat.ptr(index),
                                                            nat.ptr(count), nat.ptr(mean), nat.ptr(cov), nat.ptr(w),
                                                            nat.ptr(v)))
            if rows.value <= cap:
                break
            cap = int(rows.value)   # (the host's bound was short: once more with the size the library found)
        else:
            raise RuntimeError(f"point_statistics: {rows.value} rows do not fit the {cap} asked for")
        m = int(rows.value)
        order = np.lexsort((index[:m], slot[:m]))
        slot, index = slot[:m][order], index[:m][order]
        if pose_of_slot is not None and m:
            slot = np.asarray(list(pose_of_slot), dtype=np.int32)[slot]
        return PointStatistics(count[:m][order], mean[:m][order], cov6_to_full(cov[:m][order]),
                               w[:m][order] if eigen else None, v[:m][order] if eigen else None, slot, index)

    def cluster_points(self, radius, slots=None, min_points: int = 1, max_points=None, pose_of_slot=None):
        """Euclidean clusters of the alive stored points of the poses of `slots` (None: all), the graph taken over those
        poses alone: a clustering.Clusters in ascending (slot, index) (octl_forest_cluster_points: four kernels once the
        block index of the selection exists, one wait; nothing of the map changes).  The device gives every point the
        smallest member and the size of its component; the numbering - the distinct smallest members whose size lies in
        [min_points, max_points], ascending - is finished here.  pose_of_slot maps slots to pose numbers (None: slots
        are the pose numbers)."""
        from octreelib_amd.clustering import Clusters, _number, check_cluster_args

        r, lo, hi = check_cluster_args(radius, min_points, max_points, what="cluster")
        self.ensure_built()
        sel, n_sel, chosen = self._adjust_selection(slots)
        cap = min(int(self.n_ord), int(sum(self.slot_sizes[s] for s in chosen)))
        rows = C.c_int64(0)
        for _ in range(2):
            slot = np.empty(cap, dtype=np.int32)
            index = np.empty(cap, dtype=np.int32)
            first = np.empty(cap, dtype=np.int64)
            size = np.empty(cap, dtype=np.int32)
            self.ctx.check(self.lib.octl_forest_cluster_points(self.handle, r, nat.ptr(sel), n_sel, cap, C.byref(rows),
                                                               nat.ptr(slot), nat.ptr(index), nat.ptr(first),
                                                               nat.ptr(size)))
            if rows.value <= cap:
                break
            cap = int(rows.value)   # (the host's bound was short: once more with the size the library found)
        else:
            raise RuntimeError(f"cluster: {rows.value} rows do not fit the {cap} asked for")
        m = int(rows.value)
        order = np.lexsort((index[:m], slot[:m]))
        slot, index = slot[:m][order], index[:m][order]
        label, keys, sizes = _number(first[:m][order], size[:m][order], lo, hi)
        first_slot, first_index = (keys >> 32).astype(np.int32), (keys & 0xffffffff).astype(np.int32)
        if pose_of_slot is not None:
            names = np.asarray(list(pose_of_slot), dtype=np.int32)
            slot = names[slot] if m else slot
            first_slot = names[first_slot] if len(keys) else first_slot
        return Clusters(slot, index, label, sizes, first_slot, first_index)

    def remove_small_clusters(self, radius, min_points, slots=None) -> int:
        """Every point of the poses of `slots` (None: all) whose cluster over those poses has fewer than min_points
        members leaves the map (octl_forest_remove_small_clusters: four kernels, one compaction that also applies a
        pending RANSAC mask; clustering.small_cluster_keep_np is the rule); the scheme stays.  Returns the number of
        points removed."""
        from octreelib_amd.clustering import check_cluster_args

        r, lo, _ = check_cluster_args(radius, min_points, what="remove_small_clusters")
        self.ensure_built()
        before = self.n_ord
        sel, n_sel, _ = self._adjust_selection(slots)
        n = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_remove_small_clusters(self.handle, r, lo, nat.ptr(sel), n_sel, C.byref(n)))
        self.n_ord = n.value
        self._invalidate()
        return before - n.value

    def cell_count(self, points, cell, max_count=None, slots=None) -> np.ndarray:
        """How many stored points of the poses of `slots` (None: all) lie in the lattice cell of every query point,
        capped at max_count (None: uncapped): (n,) int32 as thinning.cell_count_np defines it (octl_forest_cell_count:
        one kernel once the block index of the selection exists).  points: a host array, or a feed.DeviceCloud of f64
        points, which is read where it lies."""
        from octreelib_amd.feed import DeviceCloud
        from octreelib_amd.query import _as_queries
        from octreelib_amd.thinning import check_cell_args

        c, max_count, _ = check_cell_args(cell, max_count)
        cap = 0 if max_count is None else max_count
        if isinstance(points, DeviceCloud):
            if np.dtype(points.dtype) != np.float64:
                raise ValueError("cell_count: a DeviceCloud of float64 points is needed (f32 queries are not "
                                 "supported)")
            points.wait()
            n = len(points)
            count = np.zeros(n, dtype=np.int32)
            lib, h = self.lib, self.ctx.handle
            out = C.c_void_p()
            self.ctx.check(lib.octl_dev_alloc(h, max(4 * n, 8), C.byref(out)))
            try:
                self.cell_count_device(points.ptr, n, c, out, max_count, slots)
                if n:
                    self.ctx.check(lib.octl_dev_download(h, nat.ptr(count), out, count.nbytes))
            finally:
                lib.octl_dev_free(h, out)
            return count
        pts = _as_queries(points)
        self.ensure_built()
        sel, n_sel, _ = self._adjust_selection(slots)
        n = len(pts)
        count = np.zeros(n, dtype=np.int32)
        # (n = 0 still goes to the library: what it refuses whatever the queries is refused for an empty scan too)
        self.ctx.check(self.lib.octl_forest_cell_count(self.handle, nat.ptr(pts), n, c, cap, nat.ptr(sel), n_sel,
                                                       nat.ptr(count)))
        return count

    def cell_count_device(self, xyz_dptr, n: int, cell, count_dptr, max_count=None, slots=None):
        """cell_count for points that are in device memory already, the (n,) int32 answer left there (pointers from
        octl_dev_alloc); enqueued on the context's stream, the host does not wait."""
        from octreelib_amd.thinning import check_cell_args

        c, max_count, _ = check_cell_args(cell, max_count)
        self.ensure_built()
        sel, n_sel, _ = self._adjust_selection(slots)
        self.ctx.check(self.lib.octl_forest_cell_count_device(self.handle, xyz_dptr, int(n), c,
                                                              0 if max_count is None else max_count, nat.ptr(sel),
                                                              n_sel, count_dptr))

    def thin(self, cell, max_per_cell=1, slots=None, among=None) -> int:
        """Voxel-grid thinning: of the points that share a lattice cell, every point of the poses of `slots` (None:
        all) that has max_per_cell or more points of the poses of `among` (None: all) before it - poses in slot order,
        rows in insertion order - leaves the map (octl_forest_thin: one kernel, one compaction that also applies a
        pending RANSAC mask; thinning.thin_keep_np is the rule); the scheme stays.  Returns the number of points
        removed."""
        from octreelib_amd.thinning import _required, check_cell_args

        c, _, m = check_cell_args(cell, None, _required(max_per_cell), what="thin")
        self.ensure_built()
        before = self.n_ord
        sel, n_sel, _ = self._adjust_selection(slots)
        asel, n_asel, _ = self._adjust_selection(among)
        n = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_thin(self.handle, c, m, nat.ptr(sel), n_sel, nat.ptr(asel), n_asel,
                                                 C.byref(n)))
        self.n_ord = n.value
        self._invalidate()
        return before - n.value

    def _raycast_args(self, max_range, min_range, surface, min_points, max_variance, origins, directions):
        from octreelib_amd.query import check_raycast_args, check_raycast_cap, normalize_directions, ray_inputs

        code, min_points, mv = check_raycast_args(surface, min_points, max_variance)
        o, d, tmin, tmax = ray_inputs(origins, normalize_directions(directions), min_range, max_range)
        if self.mode == 0:
            check_raycast_cap(tmin, tmax, float(self._cube[1]))
        return code, min_points, mv, o, d, tmin, tmax

    def raycast(self, origins, directions, max_range, min_range=0.0, slots=None, surface: str = "cube",
                min_points=None, max_variance=None):
        """What every ray hits first between min_range and max_range (octl_forest_raycast: one kernel once the block
        index - "cube" - or the pooled planes - "plane" - of the selection exist): a query.RayHits as query.raycast_np
        defines it on the directions normalised by query.normalize_directions."""
        from octreelib_amd.query import RayHits

        code, min_points, mv, o, d, tmin, tmax = self._raycast_args(max_range, min_range, surface, min_points,
                                                                   max_variance, origins, directions)
        self.ensure_built()
        if code == 1:
            self.leaf_planes(slots)    # (the table `row` names; this mirror's copy stays the device's)
        sel, n_sel, _ = self._adjust_selection(slots)
        n = len(o)
        node = np.full(n, -1, dtype=np.int32)
        t = np.full(n, np.inf, dtype=np.float64)
        row = np.full(n, -1, dtype=np.int32)
        # (n = 0 still goes to the library: what it refuses whatever the rays is refused for no rays too)
        self.ctx.check(self.lib.octl_forest_raycast(self.handle, nat.ptr(o), nat.ptr(d), nat.ptr(tmin), nat.ptr(tmax), n,
                                                    nat.ptr(sel), n_sel, code, min_points, mv, nat.ptr(node),
                                                    nat.ptr(t), nat.ptr(row)))
        return RayHits(node, t, row)

    def raycast_device(self, origins_dptr, directions_dptr, t_min_dptr, t_max_dptr, n: int, node_dptr, t_dptr, row_dptr,
                       slots=None, surface: str = "cube", min_points=None, max_variance=None):
        """raycast for rays that are in device memory already (pointers from octl_dev_alloc; the directions as the
        kernel is to see them - nothing is normalised - and t_min, t_max one per ray), the answers left there;
        enqueued on the context's stream, the host does not wait.  A ray above a grid's cap finds nothing."""
        from octreelib_amd.query import check_raycast_args

        code, min_points, mv = check_raycast_args(surface, min_points, max_variance)
        self.ensure_built()
        if code == 1:
            self.leaf_planes(slots)
        sel, n_sel, _ = self._adjust_selection(slots)
        self.ctx.check(self.lib.octl_forest_raycast_device(self.handle, origins_dptr, directions_dptr, t_min_dptr,
                                                           t_max_dptr, int(n), nat.ptr(sel), n_sel, code, min_points, mv,
                                                           node_dptr, t_dptr, row_dptr))

    def n_scheme_nodes(self) -> int:
        """Rows of the node table (the length of a RayEvidence)."""
        self.ensure_built()
        n = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_ray_evidence(self.handle, None, None, None, None, None, 0, 0, None, None,
                                                         C.byref(n)))
        return n.value

    def _evidence_args(self, origins, directions, ranges, margin, min_range, returned):
        from octreelib_amd.query import check_evidence_cap, evidence_inputs

        o, d, tmin, tfree, tend = evidence_inputs(origins, directions, ranges, margin, min_range, returned)
        if self.mode == 0:
            check_evidence_cap(tmin, tfree, tend, float(self._cube[1]))
        return o, d, tmin, tfree, tend

    def ray_evidence(self, origins, directions, ranges, margin, min_range=0.0, returned=None):
        """Rays ending in / passing through every node (octl_forest_ray_evidence: one fill, one kernel, one host
        wait): a query.RayEvidence as query.ray_evidence_np defines it on the inputs of query.evidence_inputs."""
        from octreelib_amd.query import RayEvidence

        o, d, tmin, tfree, tend = self._evidence_args(origins, directions, ranges, margin, min_range, returned)
        N = self.n_scheme_nodes()
        through, hits = np.zeros(N, dtype=np.uint32), np.zeros(N, dtype=np.uint32)
        n = C.c_int64(0)
        # (n = 0 still goes to the library: what it refuses whatever the rays is refused for no rays too)
        self.ctx.check(self.lib.octl_forest_ray_evidence(self.handle, nat.ptr(o), nat.ptr(d), nat.ptr(tmin),
                                                         nat.ptr(tfree), nat.ptr(tend), len(o), N, nat.ptr(through),
                                                         nat.ptr(hits), C.byref(n)))
        return RayEvidence(through, hits)

    def ray_evidence_device(self, origins_dptr, directions_dptr, t_min_dptr, t_free_dptr, t_end_dptr, n: int,
                            through_dptr, hits_dptr, n_nodes: int):
        """ray_evidence for rays that are in device memory already (pointers from octl_dev_alloc; the directions as
        the kernel is to see them, t_min, t_free, t_end one per ray): ADDS into the caller's n_nodes u32 counters;
        enqueued on the context's stream, the host does not wait.  A ray above a grid's cap adds nothing."""
        self.ensure_built()
        self.ctx.check(self.lib.octl_forest_ray_evidence_device(self.handle, origins_dptr, directions_dptr, t_min_dptr,
                                                                t_free_dptr, t_end_dptr, int(n), through_dptr,
                                                                hits_dptr, int(n_nodes)))

    def _carved(self, call, slots, min_through, max_hits) -> int:
        """Run one of the two carve entries; the number of points removed."""
        from octreelib_amd.query import check_carve_args

        min_through, max_hits = check_carve_args(min_through, max_hits)
        self.ensure_built()
        before = self.n_ord
        sel, n_sel, _ = self._adjust_selection(slots)
        n = C.c_int64(0)
        self.ctx.check(call(nat.ptr(sel), n_sel, min_through, max_hits, C.byref(n)))
        self.n_ord = n.value
        self._invalidate()
        return before - n.value

    def carve(self, evidence, min_through: int = 2, max_hits: int = 0, slots=None) -> int:
        """Empty every (leaf, pose) block of `slots` (None: all) whose leaf at least min_through rays passed through
        and at most max_hits ended in (octl_forest_carve: two uploads, one kernel, one compaction that also applies a
        pending RANSAC mask); the scheme stays.  Returns the number of points removed."""
        self.ensure_built()
        N = self.n_scheme_nodes()
        if len(evidence) != N:
            raise ValueError(f"carve: evidence over {len(evidence)} nodes, the map has {N} (evidence belongs to the "
                             f"scheme it was taken on)")
        through = np.ascontiguousarray(evidence.through, dtype=np.uint32)
        hits = np.ascontiguousarray(evidence.hits, dtype=np.uint32)
        return self._carved(lambda *a: self.lib.octl_forest_carve(self.handle, nat.ptr(through), nat.ptr(hits), N, *a),
                            slots, min_through, max_hits)

    def carve_device(self, through_dptr, hits_dptr, n_nodes: int, min_through: int = 2, max_hits: int = 0,
                     slots=None) -> int:
        """carve with the counters where ray_evidence_device left them."""
        return self._carved(lambda *a: self.lib.octl_forest_carve_device(self.handle, through_dptr, hits_dptr,
                                                                         int(n_nodes), *a),
                            slots, min_through, max_hits)

    def carve_rays(self, origins, directions, ranges, margin, min_range=0.0, returned=None, min_through: int = 2,
                   max_hits: int = 0, slots=None) -> int:
        """ray_evidence + carve through the device forms: the rays are uploaded once, the counters never leave the
        device.  Returns the number of points removed."""
        from octreelib_amd.query import check_carve_args

        check_carve_args(min_through, max_hits)
        o, d, tmin, tfree, tend = self._evidence_args(origins, directions, ranges, margin, min_range, returned)
        N, n = self.n_scheme_nodes(), len(o)
        lib, h = self.lib, self.ctx.handle
        rays = np.ascontiguousarray(np.concatenate([o.reshape(-1), d.reshape(-1), tmin, tfree, tend]))
        buf, cnt = C.c_void_p(), C.c_void_p()
        self.ctx.check(lib.octl_dev_alloc(h, max(rays.nbytes, 8), C.byref(buf)))
        try:
            self.ctx.check(lib.octl_dev_alloc(h, max(8 * N, 8), C.byref(cnt)))
            zeros = np.zeros(2 * N, dtype=np.uint32)
            if N:
                self.ctx.check(lib.octl_dev_upload(h, cnt, nat.ptr(zeros), zeros.nbytes))
            if n:
                self.ctx.check(lib.octl_dev_upload(h, buf, nat.ptr(rays), rays.nbytes))
            at = lambda k: C.c_void_p(buf.value + 8 * k)
            through_d, hits_d = cnt, C.c_void_p(cnt.value + 4 * N)
            self.ray_evidence_device(buf, at(3 * n), at(6 * n), at(7 * n), at(8 * n), n, through_d, hits_d, N)
            return self.carve_device(through_d, hits_d, N, min_through, max_hits, slots)
        finally:
            lib.octl_dev_free(h, buf)
            if cnt.value:
                lib.octl_dev_free(h, cnt)

    def plane_segments(self, slots=None, min_points: int = 8, max_variance=None, max_angle: float = 0.1,
                       max_offset: float = 0.05):
        """The rows of leaf_planes(slots) merged across leaf faces into connected coplanar segments
        (octl_forest_plane_segments: a size query that computes and caches on the device, then the fill): a
        query.PlaneSegments as query.plane_segments_np defines it."""
        from octreelib_amd.leaf_stats import cov6_to_full
        from octreelib_amd.query import PlaneSegments, SegmentTable, check_segment_args

        min_points, mv, cos_min, max_offset = check_segment_args(min_points, max_variance, max_angle, max_offset)
        planes = self.leaf_planes(slots)
        sel, n_sel, _ = self._adjust_selection(slots)
        mv = -1.0 if mv is None else mv
        nr, ns = C.c_int64(0), C.c_int64(0)

        def call(cap_r, cap_s, *out):
            self.ctx.check(self.lib.octl_forest_plane_segments(
                self.handle, nat.ptr(sel), n_sel, min_points, mv, cos_min, max_offset, cap_r, cap_s,
                *[nat.ptr(a) for a in out], C.byref(nr), C.byref(ns)))

        call(0, 0, *([None] * 9))
        R, S = nr.value, ns.value
        if R != len(planes):
            raise RuntimeError(f"plane_segments: {R} rows on the device, {len(planes)} in the plane table")
        neighbour = np.full((R, 6), -1, dtype=np.int32)
        label = np.full(R, -1, dtype=np.int32)
        root, n_leaves = np.empty(S, dtype=np.int32), np.empty(S, dtype=np.int32)
        count, mean, cov = np.empty(S, dtype=np.int64), np.empty((S, 3)), np.empty((S, 6))
        w, v = np.empty((S, 3)), np.empty((S, 3, 3))
        if R:
            call(R, S, neighbour, label, root, n_leaves, count, mean, cov, w, v)
        return PlaneSegments(planes, neighbour, label, SegmentTable(count, mean, cov6_to_full(cov), w, v, root, n_leaves))

    # -- registration (octreelib_amd/registration.py is the host definition of the three systems) ---------------------
    @staticmethod
    def _reg_args(transform, origin, max_variance=None, max_distance=None, huber_delta=None, nearest: bool = False):
        """(transform rows, origin, max_variance, max_distance, huber_delta) as the library takes them; nearest: the
        distance is the search radius of the two nearest-point systems (required), not own-leaf's optional gate."""
        from octreelib_amd.query import check_nearest_args
        from octreelib_amd.registration import _as_origin, as_transform

        md = check_nearest_args(1, max_distance)[1] if nearest else None
        R, t = as_transform(transform)
        T12 = np.ascontiguousarray(np.concatenate([R, t[:, None]], axis=1))
        c = np.ascontiguousarray(_as_origin(origin))
        mv = -1.0 if max_variance is None else float(max_variance)
        if not nearest:
            md = -1.0 if max_distance is None else float(max_distance)
        hd = 0.0 if huber_delta is None else float(huber_delta)
        return T12, c, mv, md, hd

    def _reg_system(self, c, call):
        """The RegistrationSystem of the 28 sums and 2 counts that call(sums pointer, counts pointer), a host form of
        the library, writes."""
        from octreelib_amd.registration import system_from_sums

        sums = np.empty(28, dtype=np.float64)
        counts = np.empty(2, dtype=np.int64)
        self.ctx.check(call(nat.ptr(sums), nat.ptr(counts)))
        return system_from_sums(sums, counts, c)

    @staticmethod
    def _reg_neighbours(slot, index, d2, pose_of_slot):
        """The (n, 1) per-point answers of a nearest-point system as query.Neighbours, the pose column named through
        pose_of_slot (None: the slots)."""
        from octreelib_amd.query import Neighbours

        count = (slot[:, 0] >= 0).astype(np.int32)
        if pose_of_slot is not None and slot.size:
            names = np.asarray(list(pose_of_slot) + [-1], dtype=np.int32)   # (-1 pads index the last entry)
            slot = names[slot]
        return Neighbours(slot, index, d2, count)

    def _align_on_device(self, points, what, prepare, system_device, accepts_device_cloud, initial, max_iterations,
                         tolerance, damping):
        """registration.align_np over one of the three systems: the scan is uploaded once - or, where accepted, is a
        feed.DeviceCloud of f64 points, read where it lies - prepare() makes the map's tables once, and every
        iteration is system_device(scan, n, T, origin, sums pointer, counts pointer) on the resident scan plus one
        download of the 28 + 2 numbers (one host wait, whatever the size of the scan); the 6x6 solve runs on the
        host."""
        from octreelib_amd.query import _as_queries
        from octreelib_amd.registration import align_np, default_origin, system_from_sums

        lib, h = self.lib, self.ctx.handle
        scan, out = C.c_void_p(), C.c_void_p()
        resident = False
        if accepts_device_cloud:
            from octreelib_amd.feed import DeviceCloud

            resident = isinstance(points, DeviceCloud)
        if resident:
            if np.dtype(points.dtype) != np.float64:
                raise ValueError(f"{what}: a DeviceCloud of float64 points is needed (f32 queries are not supported)")
            points.wait()
            n, scan = len(points), points.ptr
            pts = np.empty((n, 3), dtype=np.float64)     # (the origin of the first iteration needs the points once)
            if n:
                self.ctx.check(lib.octl_dev_download(h, nat.ptr(pts), scan, pts.nbytes))
        else:
            pts = _as_queries(points)
            n = len(pts)
        prepare()
        if not resident:
            self.ctx.check(lib.octl_dev_alloc(h, max(pts.nbytes, 8), C.byref(scan)))
        try:
            self.ctx.check(lib.octl_dev_alloc(h, 256, C.byref(out)))
            if n and not resident:
                self.ctx.check(lib.octl_dev_upload(h, scan, nat.ptr(pts), pts.nbytes))
            counts_dptr = C.c_void_p(out.value + 28 * 8)
            buf = np.empty(30, dtype=np.float64)

            def system(T, origin):
                if origin is None:
                    origin = default_origin(T, pts)
                system_device(scan, n, T, origin, out, counts_dptr)
                self.ctx.check(lib.octl_dev_download(h, nat.ptr(buf), out, buf.nbytes))
                return system_from_sums(buf[:28].copy(), buf[28:].view(np.int64), origin)

            return align_np(system, initial, max_iterations, tolerance, damping)
        finally:
            if not resident:
                lib.octl_dev_free(h, scan)    # (back to the context's pool: no hipFree on the scan path)
            if out.value:
                lib.octl_dev_free(h, out)

    def registration_system(self, points, transform=None, origin=None, slots=None, min_points: int = 8,
                            max_variance=None, max_distance=None, huber_delta=None, per_point: bool = False):
        """The point-to-plane normal equations of a scan under `transform` (octl_forest_registration_system: two
        kernels, one host wait); origin None: the centroid of the transformed scan.  per_point: the answers
        point_to_plane gives for the transformed scan come back with the system."""
        from octreelib_amd.query import _as_queries
        from octreelib_amd.registration import default_origin

        pts = _as_queries(points)
        planes = self.leaf_planes(slots)
        if origin is None:
            origin = default_origin(transform, pts)
        T12, c, mv, md, hd = self._reg_args(transform, origin, max_variance, max_distance, huber_delta)
        n = len(pts)
        node = np.empty(n, dtype=np.int32) if per_point else None
        row = np.empty(n, dtype=np.int32) if per_point else None
        res = np.empty(n, dtype=np.float64) if per_point else None
        out = self._reg_system(c, lambda sums, counts: self.lib.octl_forest_registration_system(
            self.handle, nat.ptr(pts), n, nat.ptr(T12), nat.ptr(c), int(min_points), mv, md, hd, sums, counts,
            nat.ptr(node), nat.ptr(row), nat.ptr(res)))
        if per_point:
            out.node, out.row, out.residual, out.planes = node, row, res, planes
        return out

    def registration_system_device(self, xyz_dptr, n: int, transform, origin, sys_dptr, counts_dptr, node_dptr=None,
                                   row_dptr=None, residual_dptr=None, min_points: int = 8, max_variance=None,
                                   max_distance=None, huber_delta=None):
        """registration_system against the pooled table the device holds (leaf_planes first), device pointers in and
        out (28 f64 and 2 i64); the host does not wait."""
        T12, c, mv, md, hd = self._reg_args(transform, origin, max_variance, max_distance, huber_delta)
        self.ctx.check(self.lib.octl_forest_registration_system_device(
            self.handle, xyz_dptr, int(n), nat.ptr(T12), nat.ptr(c), int(min_points), mv, md, hd, sys_dptr,
            counts_dptr, node_dptr, row_dptr, residual_dptr))

    def align(self, points, initial=None, slots=None, min_points: int = 8, max_variance=None, max_distance=None,
              huber_delta=None, max_iterations: int = 20, tolerance: float = 1e-9, damping: float = 0.0):
        """Gauss-Newton scan-to-map alignment (_align_on_device over registration_system_device): the pooled planes
        are made once; an iteration is two launches and one host wait."""
        return self._align_on_device(
            points, "align", lambda: self.leaf_planes(slots),
            lambda scan, n, T, origin, out, counts: self.registration_system_device(
                scan, n, T, origin, out, counts, None, None, None, min_points, max_variance, max_distance, huber_delta),
            False, initial, max_iterations, tolerance, damping)

    # -- point-to-point registration (registration.point_registration_system_np is the host definition) ---------------
    def point_registration_system(self, points, transform=None, origin=None, slots=None, max_distance=None,
                                  huber_delta=None, per_point: bool = False, pose_of_slot=None):
        """The point-to-point normal equations of a scan under `transform` against the nearest stored point of the
        poses of `slots` (None: all) within max_distance (octl_forest_point_registration_system: three kernels once
        the block index of the selection exists, one host wait); origin None: the centroid of the transformed scan.
        per_point: the answers nearest gives for the transformed scan with k = 1 come back with the system, the pose
        column named through pose_of_slot (None: the slots)."""
        from octreelib_amd.query import _as_queries, check_nearest_args
        from octreelib_amd.registration import default_origin

        check_nearest_args(1, max_distance)
        pts = _as_queries(points)
        if origin is None:
            origin = default_origin(transform, pts)
        T12, c, _, r, hd = self._reg_args(transform, origin, None, max_distance, huber_delta, nearest=True)
        self.ensure_built()
        sel, n_sel, _ = self._adjust_selection(slots)
        n = len(pts)
        slot = np.full((n, 1), -1, dtype=np.int32) if per_point else None
        index = np.full((n, 1), -1, dtype=np.int64) if per_point else None
        d2 = np.full((n, 1), np.inf, dtype=np.float64) if per_point else None
        # (n = 0 still goes to the library: what it refuses whatever the scan is refused for an empty one too)
        out = self._reg_system(c, lambda sums, counts: self.lib.octl_forest_point_registration_system(
            self.handle, nat.ptr(pts), n, nat.ptr(T12), nat.ptr(c), r, hd, nat.ptr(sel), n_sel, sums, counts,
            nat.ptr(slot), nat.ptr(index), nat.ptr(d2)))
        if per_point:
            out.neighbours = self._reg_neighbours(slot, index, d2, pose_of_slot)
        return out

    def point_registration_system_device(self, xyz_dptr, n: int, transform, origin, sys_dptr, counts_dptr,
                                         max_distance=None, huber_delta=None, slots=None, slot_dptr=None,
                                         index_dptr=None, d2_dptr=None):
        """point_registration_system for points that are in device memory already, device pointers in and out (28 f64
        and 2 i64; slot i32, index i64 and distance2 f64 per point, all three or none); the host does not wait."""
        T12, c, _, r, hd = self._reg_args(transform, origin, None, max_distance, huber_delta, nearest=True)
        self.ensure_built()
        sel, n_sel, _ = self._adjust_selection(slots)
        self.ctx.check(self.lib.octl_forest_point_registration_system_device(
            self.handle, xyz_dptr, int(n), nat.ptr(T12), nat.ptr(c), r, hd, nat.ptr(sel), n_sel, sys_dptr, counts_dptr,
            slot_dptr, index_dptr, d2_dptr))

    def align_points(self, points, initial=None, slots=None, max_distance=None, huber_delta=None,
                     max_iterations: int = 20, tolerance: float = 1e-9, damping: float = 0.0):
        """Gauss-Newton scan-to-map alignment against the nearest stored points (_align_on_device over
        point_registration_system_device; `points` may be a feed.DeviceCloud of f64 points): the block index is made
        once; an iteration is three launches and one host wait."""
        from octreelib_amd.query import check_nearest_args

        check_nearest_args(1, max_distance)
        return self._align_on_device(
            points, "align_points", lambda: None,
            lambda scan, n, T, origin, out, counts: self.point_registration_system_device(
                scan, n, T, origin, out, counts, max_distance, huber_delta, slots),
            True, initial, max_iterations, tolerance, damping)

    # -- nearest-point-to-plane registration (registration.nearest_plane_registration_system_np is the definition) -----
    def nearest_plane_registration_system(self, points, transform=None, origin=None, slots=None, max_distance=None,
                                          min_points: int = 8, max_variance=None, huber_delta=None,
                                          per_point: bool = False, pose_of_slot=None):
        """The point-to-plane normal equations of a scan under `transform`, every point scored against the pooled
        plane of the leaf its nearest stored point of the poses of `slots` (None: all) lies in
        (octl_forest_nearest_plane_registration_system: three kernels once the tables of the selection exist, one
        host wait); origin None: the centroid of the transformed scan.  per_point: neighbours (the answers of nearest
        with k = 1 for the transformed scan, the pose column named through pose_of_slot), node, row, residual and
        planes come back with the system."""
        from octreelib_amd.query import _as_queries, check_nearest_args
        from octreelib_amd.registration import default_origin

        check_nearest_args(1, max_distance)
        pts = _as_queries(points)
        if origin is None:
            origin = default_origin(transform, pts)
        T12, c, mv, r, hd = self._reg_args(transform, origin, max_variance, max_distance, huber_delta, nearest=True)
        planes = self.leaf_planes(slots)
        sel, n_sel, _ = self._adjust_selection(slots)
        n = len(pts)
        slot = np.full((n, 1), -1, dtype=np.int32) if per_point else None
        index = np.full((n, 1), -1, dtype=np.int64) if per_point else None
        d2 = np.full((n, 1), np.inf, dtype=np.float64) if per_point else None
        node = np.full(n, -1, dtype=np.int32) if per_point else None
        row = np.full(n, -1, dtype=np.int32) if per_point else None
        res = np.full(n, np.nan, dtype=np.float64) if per_point else None
        # (n = 0 still goes to the library: what it refuses whatever the scan is refused for an empty one too)
        out = self._reg_system(c, lambda sums, counts: self.lib.octl_forest_nearest_plane_registration_system(
            self.handle, nat.ptr(pts), n, nat.ptr(T12), nat.ptr(c), r, hd, nat.ptr(sel), n_sel, int(min_points), mv,
            sums, counts, nat.ptr(slot), nat.ptr(index), nat.ptr(d2), nat.ptr(node), nat.ptr(row), nat.ptr(res)))
        if per_point:
            out.neighbours = self._reg_neighbours(slot, index, d2, pose_of_slot)
            out.node, out.row, out.residual, out.planes = node, row, res, planes
        return out

    def nearest_plane_registration_system_device(self, xyz_dptr, n: int, transform, origin, sys_dptr, counts_dptr,
                                                 max_distance=None, min_points: int = 8, max_variance=None,
                                                 huber_delta=None, slots=None, slot_dptr=None, index_dptr=None,
                                                 d2_dptr=None, node_dptr=None, row_dptr=None, residual_dptr=None):
        """nearest_plane_registration_system against the pooled table the device holds (leaf_planes(slots) first), for
        points that are in device memory already, device pointers in and out (28 f64 and 2 i64; slot i32, index i64,
        distance2 f64, node i32, row i32 and residual f64 per point, all six or none); the host does not wait."""
        T12, c, mv, r, hd = self._reg_args(transform, origin, max_variance, max_distance, huber_delta, nearest=True)
        self.ensure_built()
        sel, n_sel, _ = self._adjust_selection(slots)
        self.ctx.check(self.lib.octl_forest_nearest_plane_registration_system_device(
            self.handle, xyz_dptr, int(n), nat.ptr(T12), nat.ptr(c), r, hd, nat.ptr(sel), n_sel, int(min_points), mv,
            sys_dptr, counts_dptr, slot_dptr, index_dptr, d2_dptr, node_dptr, row_dptr, residual_dptr))

    def align_nearest_planes(self, points, initial=None, slots=None, max_distance=None, min_points: int = 8,
                             max_variance=None, huber_delta=None, max_iterations: int = 20, tolerance: float = 1e-9,
                             damping: float = 0.0):
        """Gauss-Newton scan-to-map alignment, nearest stored point to the plane of its leaf (_align_on_device over
        nearest_plane_registration_system_device; `points` may be a feed.DeviceCloud of f64 points): the pooled planes
        and the block index are made once; an iteration is three launches and one host wait."""
        from octreelib_amd.query import check_nearest_args

        check_nearest_args(1, max_distance)
        return self._align_on_device(
            points, "align_nearest_planes", lambda: self.leaf_planes(slots),
            lambda scan, n, T, origin, out, counts: self.nearest_plane_registration_system_device(
                scan, n, T, origin, out, counts, max_distance, min_points, max_variance, huber_delta, slots),
            True, initial, max_iterations, tolerance, damping)

    # -- plane adjustment (octreelib_amd/adjustment.py is the host definition) ---------------------------------------------
    def _adjust_selection(self, slots):
        """(selection mask or None, its length, the selected slots in ascending order)"""
        if slots is None:
            return None, 0, list(range(self.n_slots))
        chosen = sorted(set(int(s) for s in slots))
        sel = np.zeros(max(self.n_slots, 1), dtype=np.uint8)[:self.n_slots]
        sel[chosen] = 1
        return np.ascontiguousarray(sel), self.n_slots, chosen

    def adjustment_origin(self) -> np.ndarray:
        """Centre of the box spanned by the scheme's root cubes (the single cube's centre): the default origin."""
        from octreelib_amd.adjustment import root_box_centre

        nd = self.nodes
        roots = np.nonzero(nd["depth"] == 0)[0] if len(nd["depth"]) else np.zeros(0, dtype=np.int64)
        return root_box_centre(nd["corner"][roots], nd["edge"][roots])

    def adjustment_system(self, transforms=None, slots=None, origin=None, min_points: int = 8, min_poses: int = 2,
                          max_variance=None, leaves: bool = False, pose_numbers=None):
        """The per-pose plane-adjustment systems at `transforms` (octl_forest_adjustment_system: the block moments
        are made once per map and selection, a call is three kernels and one host wait).  pose_numbers: the names the
        result carries for the selected slots (ascending slot order; None: the slots themselves)."""
        from octreelib_amd.adjustment import _as_origin, as_transforms, system_from_device

        self.ensure_built()
        sel, n_sel, chosen = self._adjust_selection(slots)
        S = len(chosen)
        T = np.ascontiguousarray(as_transforms(transforms, S).reshape(S, 12))
        c = np.ascontiguousarray(_as_origin(self.adjustment_origin() if origin is None else origin))
        mv = -1.0 if max_variance is None else float(max_variance)
        sums = np.zeros((S, 28), dtype=np.float64)
        counts = np.zeros((S, 2), dtype=np.int64)
        n_leaves = np.zeros(2, dtype=np.int64)
        self.ctx.check(self.lib.octl_forest_adjustment_system(
            self.handle, nat.ptr(sel), n_sel, nat.ptr(T), nat.ptr(c), int(min_points), int(min_poses), mv,
            nat.ptr(sums), nat.ptr(counts), nat.ptr(n_leaves)))
        out = system_from_device(sums, counts, n_leaves, c, chosen if pose_numbers is None else pose_numbers)
        if leaves:
            out.leaves, out.blocks = self.adjustment_tables(slots, out.pose_numbers, c)
        return out

    def adjustment_tables(self, slots=None, pose_numbers=None, origin=None):
        """(AdjustmentLeaves, BlockMoments) behind the last adjustment_system call (octl_forest_adjustment_tables)."""
        from octreelib_amd.adjustment import AdjustmentLeaves, BlockMoments

        nl, nb = C.c_int64(0), C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_adjustment_tables(self.handle, 0, None, None, None, None, None, None,
                                                              C.byref(nl), 0, None, None, None, C.byref(nb)))
        L, B = nl.value, nb.value
        node, count = np.empty(L, dtype=np.int32), np.empty(L, dtype=np.int64)
        mean, normal, lam = np.empty((L, 3)), np.empty((L, 3)), np.empty(L)
        used = np.empty(L, dtype=np.uint8)
        bnode, bslot, mom = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32), np.empty((B, 10))
        if L:
            self.ctx.check(self.lib.octl_forest_adjustment_tables(
                self.handle, L, nat.ptr(node), nat.ptr(count), nat.ptr(mean), nat.ptr(normal), nat.ptr(lam),
                nat.ptr(used), C.byref(nl), B, nat.ptr(bnode), nat.ptr(bslot), nat.ptr(mom), C.byref(nb)))
        nd = self.nodes
        anchor = nd["corner"][bnode] + (nd["edge"][bnode] / 2.0)[:, None] if B else np.empty((0, 3))
        chosen = list(range(self.n_slots)) if slots is None else sorted(set(int(x) for x in slots))
        names = chosen if pose_numbers is None else list(pose_numbers)
        pose = np.searchsorted(np.asarray(chosen, dtype=np.int64), bslot).astype(np.int32)   # (index into the selection)
        blocks = BlockMoments(bnode, pose, mom[:, 0].astype(np.int64), mom[:, 1:4].copy(), mom[:, 4:].copy(),
                              np.ascontiguousarray(anchor, dtype=np.float64), names,
                              None if origin is None else np.asarray(origin, dtype=np.float64))
        return AdjustmentLeaves(node, count, mean, normal, lam, used.astype(bool)), blocks

    def adjust(self, initial=None, slots=None, origin=None, min_points: int = 8, min_poses: int = 2,
               max_variance=None, fixed=None, max_iterations: int = 200, tolerance: float = 1e-9,
               damping: float = 0.0, pose_numbers=None):
        """Block-Jacobi plane adjustment (adjustment.adjust_np) over the device's systems: the block moments are made
        once, an iteration is three kernels, one download of S x 240 bytes and S 6x6 solves on the host."""
        from octreelib_amd.adjustment import adjust_np

        self.ensure_built()
        _, _, chosen = self._adjust_selection(slots)
        c = self.adjustment_origin() if origin is None else origin
        system = lambda T: self.adjustment_system(T, slots, c, min_points, min_poses, max_variance, False,
                                                  pose_numbers)
        return adjust_np(system, len(chosen), initial, fixed, max_iterations, tolerance, damping)

    def transform_poses(self, transforms, slots=None):
        """Move the stored rows of the poses of `slots` (None: all; ascending slot order, as adjust orders its
        result) by one rigid transform each, in place on the device (octl_forest_transform_poses: one kernel, one
        host wait).  Afterwards this is the mirror of a fresh forest that holds the same slots: no scheme, nothing
        built, voxel membership and creation order not captured yet.  A DomainError changes nothing, here or there."""
        from octreelib_amd.adjustment import as_transforms

        sel, n_sel, chosen = self._adjust_selection(slots)
        S = len(chosen)
        T = np.ascontiguousarray(as_transforms(transforms, S).reshape(S, 12))
        self.ctx.check(self.lib.octl_forest_transform_poses(self.handle, nat.ptr(sel), n_sel,
                                                            nat.ptr(T) if S else None))
        if S == 0 or sum(self.slot_sizes) == 0:
            return   # (the library's no-op: nothing moved, whatever was built stays built)
        self.epoch = 0
        self.slot_epoch = [0] * self.n_slots
        self.has_scheme = False
        self.info = None
        self._dirty = True
        self.n_ord = 0
        self.slot_voxel_keys = [None] * self.n_slots
        self._creation_codes = np.empty(0, dtype=np.int64)
        self._code_origin = None
        self._member_next = 0
        self._member_pending = []
        self._in_place = None   # (the moved store is the forest's own)
        self._invalidate()

    def remove_slots(self, slots):
        """Let go of the poses of `slots` (octl_forest_remove_poses): their blocks leave the leaf-ordered arrays in
        one compaction - a pending RANSAC mask with them - and their rows leave the store; the scheme, the voxels and
        their creation order stay.  Returns (new slot of every old slot, -1 for a removed one; alive points that
        left).  The slots that stay are renumbered densely in ascending order."""
        chosen = sorted(set(int(s) for s in slots))
        # (a forest that has been built - with a scheme or, by a read, without - and has grown since: the library
        #  would refuse; one that was never built stays unbuilt and takes the store pass alone)
        if self.has_scheme or self.info is not None:
            self.ensure_built()
        self._resolve_membership()   # (pending captures name slots as they are numbered now: behind the last build)
        new_slot = np.arange(self.n_slots, dtype=np.int32)
        if not chosen:
            return new_slot, 0
        sel = np.zeros(self.n_slots, dtype=np.uint8)
        sel[chosen] = 1
        removed = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_remove_poses(self.handle, nat.ptr(sel), self.n_slots, nat.ptr(new_slot),
                                                         C.byref(removed)))
        keep = [s for s in range(self.n_slots) if not sel[s]]
        self.slot_sizes = [self.slot_sizes[s] for s in keep]
        self.slot_epoch = [self.slot_epoch[s] for s in keep]
        self.slot_voxel_keys = [self.slot_voxel_keys[s] for s in keep]
        self._member_next -= sum(1 for s in chosen if s < self._member_next)
        self.n_slots = len(keep)
        self._in_place = None        # (the squeezed store is the forest's own)
        if self.info is not None:
            n = C.c_int64(0)
            self.ctx.check(self.lib.octl_forest_settle(self.handle, C.byref(n)))
            self.n_ord = n.value
        self._invalidate()
        return new_slot, removed.value

    def prune(self):
        """Drop the top-level voxels that hold no point any more and collapse the empty subtrees of the rest
        (octl_forest_prune; query.prune_np is the definition): a query.PruneResult.  Points, their order and a
        pending RANSAC mask are not touched.  The voxels that go leave every pose's membership and the creation order;
        the order of the rest is kept."""
        from octreelib_amd.query import PruneResult

        if self.has_scheme or self.info is not None:
            self.ensure_built()
        self._resolve_membership()   # (pending captures name voxel ranks of the table as it is now)
        built = self.info is not None and not self._dirty
        N = self.n_scheme_nodes() if built else 0
        node_map = np.empty(N, dtype=np.int32)
        old_node = np.empty(N, dtype=np.int32)
        vox_before = self.voxels if built and self.mode == 0 else None
        pi = nat.PruneInfo()
        self.ctx.check(self.lib.octl_forest_prune(self.handle, N, nat.ptr(node_map) if N else None,
                                                  nat.ptr(old_node) if N else None, C.byref(pi)))
        if pi.nodes_before != N:
            raise RuntimeError(f"prune: {pi.nodes_before} nodes on the device, {N} in the host's table")
        V = int(pi.voxels_before)
        if vox_before is not None and pi.voxels_after != V:
            gone = self._voxel_codes(vox_before[node_map[:V] < 0])
            self.slot_voxel_keys = [k if k is None or len(k) == 0 else k[~np.isin(self._voxel_codes(k), gone)]
                                    for k in self.slot_voxel_keys]
            self._creation_codes = self._creation_codes[~np.isin(self._creation_codes, gone)]
        if self.info is not None:
            self.info.n_voxels = pi.voxels_after
            self.info.n_nodes = pi.nodes_after
            self.info.n_internal = pi.internal_after
        self._invalidate()
        return PruneResult(node_map, old_node[:pi.nodes_after].copy(), int(pi.nodes_after), int(pi.voxels_after),
                           int(pi.nodes_before - pi.nodes_after), int(pi.voxels_before - pi.voxels_after),
                           int(pi.collapsed))

    def store_size(self):
        """(rows the store holds, alive rows among them, poses) as the library counts them."""
        a, b, p = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self.ctx.check(self.lib.octl_forest_store_size(self.handle, C.byref(a), C.byref(b), C.byref(p)))
        return a.value, b.value, p.value

    @property
    def perm(self) -> np.ndarray:
        """perm[i] = index (in the concatenation of all pose clouds, slot order) of the point at
        storage position i."""
        if self._perm is None:
            self.ensure_built()
            n = C.c_int64(0)
            self.ctx.check(self.lib.octl_forest_get_perm(self.handle, 0, None, C.byref(n)))
            p = np.empty(n.value, dtype=np.int64)
            self.ctx.check(self.lib.octl_forest_get_perm(self.handle, n.value, nat.ptr(p), C.byref(n)))
            self._perm = p
        return self._perm

    # -- counters (reference: octree.py:144-175, octree_manager.py:132-159, grid.py:343-362) ---
    def _slot_counts(self, slot: int):
        """(points, non-empty leaves) of a slot, reduced on the device (no table download)."""
        self.ensure_built()
        if self._counts is None:
            self._counts = {}
        if slot not in self._counts:
            a, b = C.c_int64(0), C.c_int64(0)
            self.ctx.check(self.lib.octl_forest_slot_counts(self.handle, int(slot), C.byref(a), C.byref(b)))
            self._counts[slot] = (a.value, b.value)
        return self._counts[slot]

    def n_points(self, slot: int) -> int:
        return self._slot_counts(slot)[0]

    def n_leaves(self, slot: int) -> int:
        return self._slot_counts(slot)[1]

    def internal_per_voxel(self) -> np.ndarray:
        self.ensure_built()
        if self._internal is None:
            n = C.c_int64(0)
            self.ctx.check(self.lib.octl_forest_internal_per_voxel(self.handle, 0, None, C.byref(n)))
            out = np.zeros(n.value, dtype=np.int32)
            if n.value:
                self.ctx.check(self.lib.octl_forest_internal_per_voxel(self.handle, n.value, nat.ptr(out), C.byref(n)))
            self._internal = out.astype(np.int64)
        return self._internal

    def slot_voxel_ranks(self, slot: int) -> np.ndarray:
        """Current voxel ranks of the voxels the slot was inserted into (lexicographic)."""
        self.ensure_built()
        self._resolve_membership()
        keys = self.slot_voxel_keys[slot]
        if keys is None or len(keys) == 0:
            return np.empty(0, dtype=np.int64)
        # the packed codes order like the (x, y, z) rows: one searchsorted over int64
        return np.searchsorted(self._voxel_codes(self.voxels), self._voxel_codes(keys)).astype(np.int64)

    def n_nodes(self, slot: int) -> int:
        ranks = self.slot_voxel_ranks(slot)
        if len(ranks) == 0:
            return 0
        return int((1 + 8 * self.internal_per_voxel()[ranks]).sum())

    # -- masks ------------------------------------------------------------------------------
    def apply_host_mask(self, mask: np.ndarray):
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        n = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_apply_host_mask(self.handle, nat.ptr(mask), len(mask), C.byref(n)))
        self.n_ord = n.value
        self._invalidate()

    def filter_count(self, slots, lo: int, hi: int):
        """Empty every leaf of the given slots whose point count is outside [lo, hi] (device)."""
        self.ensure_built()
        sel = np.zeros(max(self.n_slots, 1), dtype=np.uint8)
        sel[list(slots)] = 1
        n = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_filter_count(self.handle, nat.ptr(sel), self.n_slots, int(lo),
                                                         int(min(hi, (1 << 63) - 1)), C.byref(n)))
        self.n_ord = n.value
        self._invalidate()

    def set_contents(self, blk_node, blk_slot, blk_size, xyz):
        """Replace the contents of the leaves, scheme kept (map_leaf_points with a transforming function)."""
        self.ensure_built()
        node = np.ascontiguousarray(blk_node, dtype=np.int32)
        slot = np.ascontiguousarray(blk_slot, dtype=np.int32)
        size = np.ascontiguousarray(blk_size, dtype=np.int32)
        pts = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        assert int(size.sum()) == len(pts)
        self.ctx.check(self.lib.octl_forest_set_contents(self.handle, len(node), nat.ptr(node), nat.ptr(slot),
                                                         nat.ptr(size), nat.ptr(pts)))
        self.n_ord = len(pts)
        self._in_place = None
        for s in range(self.n_slots):
            self.slot_sizes[s] = int(size[slot == s].sum())
        self._invalidate()

    def apply_device_mask(self):
        # (octl_forest_apply_mask_async: the compaction is enqueued, its counts are booked when somebody asks -
        #  the reference's map_leaf_points_cuda_ransac returns nothing, grid.py:124-215)
        self.ctx.check(self.lib.octl_forest_apply_mask_async(self.handle))
        self._n_ord_pending = True
        self._invalidate()

    @property
    def n_ord(self) -> int:
        """Points in the leaf-ordered arrays (after an apply_mask whose count is still on its way: waits for it)."""
        if self._n_ord_pending:
            n = C.c_int64(0)
            self.ctx.check(self.lib.octl_forest_settle(self.handle, C.byref(n)))
            self._n_ord = n.value
            self._n_ord_pending = False
        return self._n_ord

    @n_ord.setter
    def n_ord(self, value: int):
        self._n_ord = int(value)
        self._n_ord_pending = False

    def device_mask(self) -> np.ndarray:
        n = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_get_mask(self.handle, 0, None, C.byref(n)))
        m = np.empty(n.value, dtype=np.uint8)
        self.ctx.check(self.lib.octl_forest_get_mask(self.handle, n.value, nat.ptr(m), C.byref(n)))
        return m

    # -- RANSAC -----------------------------------------------------------------------------
    def ransac_all(self, poses_per_batch: int, hypotheses: np.ndarray, threshold: float):
        self.ensure_built()
        hyp = np.ascontiguousarray(hypotheses, dtype=np.float64)
        e0 = np.ascontiguousarray(np.asarray(self.slot_epoch, dtype=np.int32))
        self.ctx.check(
            self.lib.octl_forest_ransac_all(
                self.handle, int(poses_per_batch), nat.ptr(e0), self.n_slots, nat.ptr(hyp),
                hyp.shape[0], hyp.shape[1], float(threshold),
            )
        )

    def ransac_blocks(self, block_order: np.ndarray, hypotheses: np.ndarray, threshold: float,
                      details=False):
        self.ensure_built()
        order = np.ascontiguousarray(block_order, dtype=np.int32)
        hyp = np.ascontiguousarray(hypotheses, dtype=np.float64)
        nb = len(order)
        plane = np.empty((nb, 4), dtype=np.float32) if details else None
        count = np.empty(nb, dtype=np.int32) if details else None
        index = np.empty(nb, dtype=np.int32) if details else None
        self.ctx.check(
            self.lib.octl_forest_ransac(
                self.handle, nat.ptr(order), nb, nat.ptr(hyp), hyp.shape[0], hyp.shape[1],
                float(threshold), nat.ptr(plane), nat.ptr(count), nat.ptr(index),
            )
        )
        return plane, count, index


def _node_paths(nd):
    """Child-digit path (tuple) of every scheme node."""
    n = len(nd["parent"])
    paths = [()] * n
    order = np.argsort(nd["depth"], kind="stable")
    par, fc = nd["parent"], nd["first_child"]
    for i in order.tolist():
        p = par[i]
        if p >= 0:
            paths[i] = paths[p] + (int(i - fc[p]),)
    return paths
