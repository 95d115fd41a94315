"""Host-side mirror of the reference's scene data model (inputs to the hot path).

Names follow the reference: `Scene{objects}` / `Object{geometry, material}` (core/src/scene.rs:33-45),
`Geometry::{Plane, Sphere, Grid}` (:9-13), `Material::{Diffuse, Metal, Emission}` (core/src/lib.rs:21-26),
`Mesh{triangles, bounding_box}` + `bake_transform` (core/src/geometry/mesh.rs:10-56) and
`AccGrid::build_from_mesh` (core/src/geometry/acc_grid.rs:36-83).  No arithmetic of the per-pixel
path lives here; `flatten()` turns a Scene into the POD arrays of include/raymond_hip.h.
"""
import ctypes as C

import numpy as np

from . import abi


# ---------------------------------------------------------------- Material (core/src/lib.rs:21-26)
class Material:
    def __init__(self, kind, color, roughness=0.0, aux=(0.0, 0.0, 0.0, 0.0, 0.0)):
        self.kind = kind
        self.color = tuple(float(c) for c in color)
        self.roughness = float(roughness)
        self.aux = tuple(float(a) for a in aux)

    @staticmethod
    def Diffuse(color, roughness):
        return Material(abi.RMD_MAT_DIFFUSE, color, roughness)

    @staticmethod
    def Metal(color, roughness):
        return Material(abi.RMD_MAT_METAL, color, roughness)

    @staticmethod
    def Emission(e, v2=(1.0, 1.0, 1.0), f1=0.0, f2=0.0):
        return Material(abi.RMD_MAT_EMISSION, e, 0.0, (v2[0], v2[1], v2[2], f1, f2))


# ---------------------------------------------------------------- Geometry (core/src/scene.rs:9-13)
class Plane:  # core/src/geometry/primitives/plane.rs:5-8
    def __init__(self, origin, normal):
        self.origin = tuple(float(c) for c in origin)
        self.normal = tuple(float(c) for c in normal)


class Sphere:  # core/src/geometry/primitives/sphere.rs:5-8
    def __init__(self, origin, radius):
        self.origin = tuple(float(c) for c in origin)
        self.radius = float(radius)


class Mesh:
    """Triangle soup: tri_pos / tri_nrm are (N, 9) float64 (v0 v1 v2 / n0 n1 n2).  mesh.rs:10-13."""

    def __init__(self, tri_pos, tri_nrm):
        self.tri_pos = np.ascontiguousarray(tri_pos, dtype=np.float64).reshape(-1, 9)
        self.tri_nrm = np.ascontiguousarray(tri_nrm, dtype=np.float64).reshape(-1, 9)
        assert self.tri_pos.shape == self.tri_nrm.shape

    @staticmethod
    def load_ply(path):
        """Mesh::load_ply (mesh.rs:58-121): ASCII PLY; only `element vertex N` is read from the header, vertex lines are
        `x y z nx ny nz [s t]`, face lines `3 i j k`; faces with another vertex count are dropped (:116).  A malformed file
        raises (the reference panics on its unwrap()s)."""
        with open(path) as f:
            lines = f.read().splitlines()  # like Rust's str::lines(): no trailing empty element
        it = iter(lines)
        n_vertices = 0
        for line in it:
            tok = line.split()
            if not tok:
                raise ValueError("load_ply: empty header line")
            if tok[0] == "element" and len(tok) > 2 and tok[1] == "vertex":
                n_vertices = int(tok[2])
            elif tok[0] == "end_header":
                break
        verts = []
        for _ in range(n_vertices):
            v = [float(t) for t in next(it).split()]
            verts.append((v[0:3], v[3:6]))
        pos, nrm = [], []
        for line in it:
            v = [int(t) for t in line.split()]
            if not v:
                raise ValueError("load_ply: empty face line")  # values[0] panics in the reference
            if v[0] != 3:
                continue
            tri = [verts[i] for i in v[1:4]]
            pos.append(sum((t[0] for t in tri), []))
            nrm.append(sum((t[1] for t in tri), []))
        return Mesh(np.array(pos, dtype=np.float64).reshape(-1, 9), np.array(nrm, dtype=np.float64).reshape(-1, 9))

    def bake_transform(self, translate):
        """mesh.rs:48-56: position += translate for every vertex (bounds are recomputed by the grid build)."""
        t = np.asarray(translate, dtype=np.float64)
        self.tri_pos = self.tri_pos + np.tile(t, 3)[None, :]

    def __len__(self):
        return self.tri_pos.shape[0]


class AccGrid:
    """acc_grid.rs:27-33 in the compact layout of rmd_grid_desc (u32 cells / mapping_table)."""

    def __init__(self, bbox_min, bbox_max, resolution, cell_size, cells, mapping_table, tri_pos, tri_nrm):
        self.bbox_min = np.asarray(bbox_min, dtype=np.float64).copy()
        self.bbox_max = np.asarray(bbox_max, dtype=np.float64).copy()
        self.resolution = np.asarray(resolution, dtype=np.uint32).copy()
        self.cell_size = np.asarray(cell_size, dtype=np.float64).copy()
        self.cells = np.ascontiguousarray(cells, dtype=np.uint32)
        self.mapping_table = np.ascontiguousarray(mapping_table, dtype=np.uint32)
        self.tri_pos = np.ascontiguousarray(tri_pos, dtype=np.float64).reshape(-1, 9)
        self.tri_nrm = np.ascontiguousarray(tri_nrm, dtype=np.float64).reshape(-1, 9)

    @staticmethod
    def from_desc(desc):
        """Deep-copies the arrays a (library- or oracle-owned) rmd_grid_desc points at."""
        nt = int(desc.n_tris)
        return AccGrid(
            list(desc.bbox_min),
            list(desc.bbox_max),
            list(desc.resolution),
            list(desc.cell_size),
            np.ctypeslib.as_array(desc.cells, shape=(int(desc.n_cells),)).copy(),
            np.ctypeslib.as_array(desc.mapping_table, shape=(int(desc.n_mapping),)).copy(),
            np.ctypeslib.as_array(desc.tri_pos, shape=(nt * 9,)).copy(),
            np.ctypeslib.as_array(desc.tri_nrm, shape=(nt * 9,)).copy(),
        )

    @staticmethod
    def build_from_mesh(mesh, ctx=None):
        """AccGrid::build_from_mesh through the product's host builder (rmd_grid_build_from_mesh), or on the GPU of
        `ctx` (rmd_grid_build_from_mesh_gpu) — both give byte-identical tables."""
        from . import lib as _lib

        L = _lib.load()
        handle = C.c_void_p()
        pos, nrm = mesh.tri_pos.ctypes.data_as(C.c_void_p), mesh.tri_nrm.ctypes.data_as(C.c_void_p)
        if ctx is None:
            _lib.check(L.rmd_grid_build_from_mesh(pos, nrm, len(mesh), C.byref(handle)))
        else:
            _lib.check(L.rmd_grid_build_from_mesh_gpu(ctx.handle, pos, nrm, len(mesh), C.byref(handle)), ctx.handle)
        try:
            desc = abi.GridDesc()
            _lib.check(L.rmd_grid_build_describe(handle, C.byref(desc)))
            return AccGrid.from_desc(desc)
        finally:
            L.rmd_grid_build_destroy(handle)

    def desc(self):
        d = abi.GridDesc()
        d.bbox_min[:] = self.bbox_min.tolist()
        d.bbox_max[:] = self.bbox_max.tolist()
        d.resolution[:] = [int(v) for v in self.resolution]
        d.cell_size[:] = self.cell_size.tolist()
        d.cells = self.cells.ctypes.data_as(C.POINTER(C.c_uint32))
        d.n_cells = self.cells.size
        d.mapping_table = self.mapping_table.ctypes.data_as(C.POINTER(C.c_uint32))
        d.n_mapping = self.mapping_table.size
        d.tri_pos = self.tri_pos.ctypes.data_as(C.POINTER(C.c_double))
        d.tri_nrm = self.tri_nrm.ctypes.data_as(C.POINTER(C.c_double))
        d.n_tris = self.tri_pos.shape[0]
        return d


class Grid:  # Geometry::Grid(Arc<AccGrid>)
    def __init__(self, acc_grid):
        self.grid = acc_grid


class Object:  # core/src/scene.rs:33-37
    def __init__(self, geometry, material):
        self.geometry = geometry
        self.material = material


class Scene:  # core/src/scene.rs:42-52
    def __init__(self):
        self.objects = []

    def flatten(self):
        """-> (objects: (abi.Object * n), grids: (abi.GridDesc * g), keepalive list).  Object order is kept."""
        grids = []
        objs = (abi.Object * max(1, len(self.objects)))()
        for i, o in enumerate(self.objects):
            r = objs[i]
            g = o.geometry
            if isinstance(g, Plane):
                r.geometry_kind = abi.RMD_GEOM_PLANE
                r.origin[:] = g.origin
                r.normal[:] = g.normal
            elif isinstance(g, Sphere):
                r.geometry_kind = abi.RMD_GEOM_SPHERE
                r.origin[:] = g.origin
                r.radius = g.radius
            elif isinstance(g, Grid):
                r.geometry_kind = abi.RMD_GEOM_GRID
                if g.grid not in grids:
                    grids.append(g.grid)
                r.grid_index = grids.index(g.grid)
            else:
                raise TypeError("unknown geometry %r" % (g,))
            m = o.material
            r.material.kind = m.kind
            r.material.color[:] = m.color
            r.material.roughness = m.roughness
            r.material.emission_aux[:] = m.aux
        descs = (abi.GridDesc * max(1, len(grids)))()
        for i, g in enumerate(grids):
            descs[i] = g.desc()
        return objs, len(self.objects), descs, len(grids), grids


# ---------------------------------------------------------------- Settings (src/trace.rs:32-55)
class Transform:  # src/transform.rs:4-14
    def __init__(self, position=(0.0, 0.0, 0.0)):
        self.position = tuple(float(c) for c in position)

    @staticmethod
    def identity():
        return Transform()


class CameraSettings:
    def __init__(self, backbuffer_width, backbuffer_height, fov_vert, transform=None, focal_length=2.5, aperture_radius=0.0):
        self.backbuffer_width = int(backbuffer_width)
        self.backbuffer_height = int(backbuffer_height)
        self.fov_vert = float(fov_vert)
        self.transform = transform or Transform.identity()
        self.focal_length = float(focal_length)
        self.aperture_radius = float(aperture_radius)

    def pod(self):
        c = abi.Camera()
        c.backbuffer_width = self.backbuffer_width
        c.backbuffer_height = self.backbuffer_height
        c.fov_vert = self.fov_vert
        c.position[:] = self.transform.position
        c.focal_length = self.focal_length
        c.aperture_radius = self.aperture_radius
        return c


class Settings:
    """src/trace.rs:42-55 plus the RNG seed the reference lacks."""

    def __init__(self, camera_settings, sample_count, tile_size=(32, 32), bounce_limit=5, samples_per_iteration=0,
                 worker_count=None, seed=0x5EED0001, use_dof=False, trace_black_paths=False, end_black_paths=False, adaptive_threshold=0.0,
                 adaptive_floor=1e-3, denoise=False, denoise_radius=10, denoise_patch=3, denoise_k=0.45, denoise_alpha=1.0,
                 denoise_features=False, denoise_feature_k=1.0, denoise_feature_tau=1e-2, denoise_dual=False, adaptive_denoised_threshold=0.0,
                 adaptive_min_samples=32, denoise_dual_features=False, denoise_dual_select=False, denoise_atrous=False,
                 denoise_atrous_levels=5, denoise_atrous_k=3.0, denoise_dual_atrous=False, denoise_dual_atrous_region=False, preview_every=0,
                 preview_exposure=1.0, preview_gamma=2.2, preview_denoise=False, progress_tiles=True, preview_auto_exposure=False,
                 auto_exposure_percentile=0.99, auto_exposure_target=0.8, denoise_feature_slope=0.0,
                 denoise_atrous_slope=0.0, despike=False, despike_radius=2, despike_rank=2, despike_k=6.0, despike_ratio=2.0, despike_floor=0.0,
                 adaptive_measure="channel_max", adaptive_display_threshold=0.0, adaptive_display_exposure=1.0, adaptive_display_gamma=2.2,
                 adaptive_display_floor=1.0 / 255.0, adaptive_display_auto_exposure=False, adaptive_denoised_display_threshold=0.0, despike_dual=False):
        self.camera_settings = camera_settings
        self.sample_count = int(sample_count)
        self.tile_size = (int(tile_size[0]), int(tile_size[1]))
        self.bounce_limit = int(bounce_limit)
        self.samples_per_iteration = int(samples_per_iteration)
        self.worker_count = worker_count  # number of GPUs (contexts) here; None = 1
        self.seed = int(seed)
        # The reference's loop always calls the pinhole generate_primary_ray (src/trace.rs:199) whatever
        # camera_settings.aperture_radius holds; use_dof=True opts into generate_primary_ray_with_dof (:335-360).
        self.use_dof = bool(use_dof)
        # A path whose throughput has become exactly (0, 0, 0) (raymond_hip.h: RMD_RENDER_*_BLACK_PATHS).  Default: reference-identical —
        # ended in scenes without grids (provably the same samples), traced on in scenes with a grid (a later mesh vertex may make the
        # reference's sample 0 x NaN = NaN).  end_black_paths=True ends them in grid scenes too; trace_black_paths=True never ends one.
        self.trace_black_paths = bool(trace_black_paths)
        self.end_black_paths = bool(end_black_paths)
        # Adaptive tile sampling (an extension; 0.0 = off, the reference's behaviour): after every progressive pass a tile whose relative standard
        # error (raymond_hip.h: rmd_tile_error, with `adaptive_floor` as its floor) is at most `adaptive_threshold` is finished at the samples it has.
        self.adaptive_threshold = float(adaptive_threshold)
        self.adaptive_floor = float(adaptive_floor)
        # What the adaptive_threshold check compares with the threshold: "channel_max", rmd_tile_error — the worst channel of the worst pixel —, or one
        # rmd_tile_luma_error call's tile_rms ("luma_tile": the RMS standard error of the tile's luminance over the tile's mean luminance) or pixel_rms
        # ("luma_pixel": the RMS of the pixels' relative luminance errors), both with `adaptive_floor` as the floor.  The three thresholds are not comparable
        # numbers.  Checked whether or not adaptive sampling is on; no effect on the dual loop, and refused with denoise_dual.
        self.adaptive_measure = adaptive_measure
        # Adaptive sampling by the DISPLAYED error (an extension; 0 = off; in place of adaptive_threshold, needs samples_per_iteration > 0): the check is one
        # rmd_tile_weighted_error call over the live tiles under rmd_display_weights' table — every pixel's luminance variance times the squared slope of the
        # tone curve (1 - exp(-y exposure))^(1 / gamma) at its luminance — and a tile whose rms is at most the threshold is finished at the samples it has.
        # The threshold is a fraction of the display's full scale: 1 / 255 is one 8-bit level.  adaptive_display_floor: luminances that display below it take
        # the slope at it (the cap that keeps the weight finite).  adaptive_display_auto_exposure: every check first takes the exposure its own histogram of
        # the whole frame asks for (auto_exposure_percentile, auto_exposure_target) in place of adaptive_display_exposure.  Refused with adaptive_threshold,
        # with an adaptive_measure other than "channel_max" and with denoise_dual.
        self.adaptive_display_threshold = float(adaptive_display_threshold)
        self.adaptive_display_exposure = float(adaptive_display_exposure)
        self.adaptive_display_gamma = float(adaptive_display_gamma)
        self.adaptive_display_floor = float(adaptive_display_floor)
        self.adaptive_display_auto_exposure = bool(adaptive_display_auto_exposure)
        self.check_adaptive()
        # Denoising (an extension; False = off): TaskHandle.await_() returns the assembled frame filtered by rmd_denoise (raymond_hip.h) with
        # these parameters; render_tiled then renders with second moments.
        self.denoise = bool(denoise)
        self.denoise_radius = denoise_radius
        self.denoise_patch = denoise_patch
        self.denoise_k = float(denoise_k)
        self.denoise_alpha = float(denoise_alpha)
        # Feature-guided denoising (an extension of the extension; False = off): await_() also renders the finished tiles' first-hit features
        # (rmd_render_features) and filters with rmd_denoise_guided, k_f = denoise_feature_k and tau = denoise_feature_tau (defaults: the best of the
        # sweep in DESIGN.md section 12).  Needs denoise.
        self.denoise_features = bool(denoise_features)
        self.denoise_feature_k = float(denoise_feature_k)
        self.denoise_feature_tau = float(denoise_feature_tau)
        # The feature-slope term of the guided non-local-means filters (0.0 = off: no frame, message or launch changes): the number of pixels of a
        # feature's local slope that is not an edge (raymond_hip.h: rmd_denoise_guided_slope; DESIGN.md section 21 — 3 is the value to start from).  When
        # set, whichever of denoise_features, denoise_dual_features (await_() and the adaptive check's region call) and denoise_dual_select's guided
        # candidate is on makes its _slope call with it.  Needs one of them; the a-trous filters take the term through denoise_atrous_slope, a setting of
        # its own, and are refused here.
        self.denoise_feature_slope = float(denoise_feature_slope)
        # The same term in the guided a-trous filters (0.0 = off: no frame, message or launch changes; raymond_hip.h: rmd_denoise_atrous_slope; DESIGN.md
        # section 22 — 3 is the value to start from).  When set, every call of a guided a-trous filter is its _slope call with it: await_() with denoise_atrous
        # + denoise_features or denoise_dual_atrous + denoise_dual_features, the adaptive check (its region form with denoise_dual_atrous_region) and a
        # filtered FramePreview when it is guided.  Needs one of those two pairs.
        self.denoise_atrous_slope = float(denoise_atrous_slope)
        # Dual-buffer denoising (an extension of the extension; False = off): a tile's passes go alternately into two half buffers A (even passes,
        # counted from 0) and B (odd ones), and await_() returns rmd_denoise_dual's frame: each half filtered with the other's weights.  Needs
        # denoise and samples_per_iteration > 0; one device only.
        self.denoise_dual = bool(denoise_dual)
        # Adaptive sampling by the FILTERED frame's error (0.0 = off; needs denoise_dual, excludes adaptive_threshold > 0): after every even pass
        # that leaves live tiles with at least `adaptive_min_samples` samples, a live tile whose rmd_tile_error_dual — an absolute RMS in linear
        # radiance that reads low (raymond_hip.h) — is at most the threshold is finished at the samples it has.
        self.adaptive_denoised_threshold = float(adaptive_denoised_threshold)
        self.adaptive_min_samples = adaptive_min_samples
        # Adaptive sampling by the DISPLAYED error of the filtered frame (0.0 = off; needs denoise_dual and samples_per_iteration > 0, excludes
        # adaptive_denoised_threshold > 0 and adaptive_threshold > 0): the same checks at the same passes, but after the filter call one
        # rmd_tile_weighted_error_dual call over the live tiles — the filter's error image weighted, by the filtered frame's luminance, under
        # rmd_display_weights' table at adaptive_display_exposure, adaptive_display_gamma and adaptive_display_floor (adaptive_display_auto_exposure: at the
        # exposure every check's own histogram of the whole frame's raw sums asks for) — and a tile whose rms is at most the threshold is finished.  The
        # threshold is a fraction of the display's full scale: 1 / 255 is one 8-bit level.
        self.adaptive_denoised_display_threshold = float(adaptive_denoised_display_threshold)
        # Feature weights in the dual-buffer filter (False = off; needs denoise_dual): the filter is rmd_denoise_dual_guided, with the first-hit
        # features at count_a + count_b samples per tile, k_f = denoise_feature_k and tau = denoise_feature_tau; the adaptive check is its region form.
        self.denoise_dual_features = bool(denoise_dual_features)
        # Per-pixel choice among dual-buffer filters (False = off; needs denoise_dual): await_() renders the finished tiles' features as
        # denoise_dual_features does and returns rmd_denoise_dual_select's frame at select_candidates() with both windows 2.  The adaptive check is untouched.
        self.denoise_dual_select = bool(denoise_dual_select)
        # The fast filter for previews (False = off; needs denoise, excludes denoise_dual): await_() returns rmd_denoise_atrous's frame at
        # denoise_atrous_levels (0..8) and k = denoise_atrous_k with denoise_alpha — guided by the first-hit features when denoise_features is on,
        # with denoise_feature_k and denoise_feature_tau.  denoise_radius, denoise_patch and denoise_k are then not used.
        self.denoise_atrous = bool(denoise_atrous)
        self.denoise_atrous_levels = denoise_atrous_levels
        self.denoise_atrous_k = float(denoise_atrous_k)
        # The fast filter in the dual-buffer loop (False = off; needs denoise_dual, excludes denoise_dual_select): await_() returns
        # rmd_denoise_atrous_dual's frame at denoise_atrous_levels, denoise_atrous_k and denoise_alpha — guided when denoise_dual_features is on, with
        # denoise_feature_k and denoise_feature_tau — and the adaptive check is that call on the whole frame.
        self.denoise_dual_atrous = bool(denoise_dual_atrous)
        # The region form in that check (False = off; needs denoise_dual_atrous): the check calls rmd_denoise_atrous_dual_region over the live tiles, which
        # gives their pixels the whole-frame call's bytes at a cost that follows their dilated area.  No message and no output changes; await_() is untouched.
        self.denoise_dual_atrous_region = bool(denoise_dual_atrous_region)
        self.check_denoise()
        # Frame previews during a progressive render (an extension; 0 = off): after every preview_every-th pass that leaves the render unfinished — the
        # passes after which TileProgressed is sent — one Message.FramePreview follows that pass's TileProgressed messages: the whole frame as (H, W, 3)
        # uint8, every tile resolved and tone-mapped on its device at its own sample count (rmd_resolve_tonemap_tiles) with preview_exposure and
        # preview_gamma.  Needs samples_per_iteration > 0.
        self.preview_every = preview_every
        self.preview_exposure = float(preview_exposure)
        self.preview_gamma = float(preview_gamma)
        # The preview is the fast filter's frame instead of the raw means (False = off; needs preview_every, one device only), at denoise_atrous_levels,
        # denoise_atrous_k and denoise_alpha: rmd_denoise_atrous on the sums and sums of squares — the passes then render with second moments, as they do
        # for denoise —, in the dual-buffer loop rmd_denoise_atrous_dual, guided by the feature buffers when the loop already keeps them (a half without
        # samples, after a first pass, leaves that filter nothing to cross-weight with).  Its means are resolved at count 1.
        self.preview_denoise = bool(preview_denoise)
        # False: no TileProgressed message is made and nothing is downloaded for one; an adaptive render's TileFinished messages stay, the data of
        # converged tiles coming through download_tiles of those tiles only.
        self.progress_tiles = bool(progress_tiles)
        # Automatic exposure for the previews (False = off; needs preview_every): every preview first takes the luminance histogram of exactly the buffers,
        # rects and counts its rmd_resolve_tonemap_tiles call is about to use (rmd_luminance_histogram_tiles; several devices' histograms are added), and
        # the exposure that puts the auto_exposure_percentile of luminance at auto_exposure_target before gamma (rmd_exposure_from_histogram) replaces
        # preview_exposure in that call.  The message carries it as Message.FramePreview's `exposure`.  0.99 and 0.8 are values to start from.
        self.preview_auto_exposure = bool(preview_auto_exposure)
        self.auto_exposure_percentile = float(auto_exposure_percentile)
        self.auto_exposure_target = float(auto_exposure_target)
        self.check_preview()
        # Firefly rejection in front of everything that reads the moments (an extension; False = off: no buffer, launch or copy is added).  await_()
        # despikes the assembled sums and sums of squares on the first device (raymond_hip.h: rmd_despike, at despike_radius, despike_rank, despike_k,
        # despike_ratio and despike_floor) before the plain divide, denoise, denoise_features or denoise_atrous; render_tiled then renders with second
        # moments, as for denoise.  The adaptive_threshold check despikes all tiles at their current counts into two spare buffers and runs rmd_tile_error on
        # those (one device only); the sums the passes add to, the TileFinished / TileProgressed data and the previews stay the raw sums.  Refused with
        # denoise_dual, whose halves despike_dual (below) despikes.  2, 2, 6, 2 and 0 are values to start from.
        self.despike = bool(despike)
        self.despike_radius = despike_radius
        self.despike_rank = despike_rank
        self.despike_k = float(despike_k)
        self.despike_ratio = float(despike_ratio)
        self.despike_floor = float(despike_floor)
        # Firefly rejection for the two halves of the dual-buffer paths (an extension; False = off: no buffer, launch or copy is added; needs denoise_dual).
        # It reads despike_radius, despike_rank, despike_k, despike_ratio and despike_floor (raymond_hip.h: rmd_despike_dual).  await_()
        # despikes the assembled halves on its device before whichever dual filter the settings choose; in the dual loop every call of the dual filter — the
        # adaptive check and the filtered preview — reads despiked copies, four spare buffers filled once per pass by one call over the whole frame, finished
        # tiles at the counts they finished with and live tiles at n_A / n_B.  The sums the passes add to, the TileFinished / TileProgressed data, raw
        # previews and the auto-exposure histogram stay the raw sums.  `despike` itself stays refused with denoise_dual.
        self.despike_dual = bool(despike_dual)
        self.check_despike()

    def despike_keywords(self):
        """render.despike's parameters from the settings."""
        return dict(radius=self.despike_radius, rank=self.despike_rank, k=self.despike_k, ratio=self.despike_ratio, floor=self.despike_floor)

    def check_despike(self, n_devices=1):
        """Raises ValueError for despike settings rmd_despike refuses (checked whether or not despike is on) or render_tiled cannot follow on `n_devices`."""
        v = self.despike_radius
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= abi.DESPIKE_MAX_RADIUS:
            raise ValueError("despike_radius must be an integer in [1, %d]" % abi.DESPIKE_MAX_RADIUS)
        v = self.despike_rank
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= (2 * self.despike_radius + 1) ** 2 - 2:
            raise ValueError("despike_rank must be an integer in [0, (2 * despike_radius + 1)^2 - 2]")
        if not (self.despike_k >= 0.0 and np.isfinite(self.despike_k)):
            raise ValueError("despike_k must be finite and >= 0")
        if not (self.despike_ratio >= 1.0 and np.isfinite(self.despike_ratio)):
            raise ValueError("despike_ratio must be finite and >= 1")
        if not (self.despike_floor >= 0.0 and np.isfinite(self.despike_floor)):
            raise ValueError("despike_floor must be finite and >= 0")
        if self.despike and self.denoise_dual:
            raise ValueError("despike cannot be combined with denoise_dual: the halves are not yet despiked")
        if self.despike and self.adaptive_threshold > 0.0 and n_devices != 1:
            raise ValueError("despike with adaptive_threshold renders on one device: the window crosses the tiles that several devices would own")
        if self.despike and self.adaptive_display_threshold > 0.0 and n_devices != 1:
            raise ValueError("despike with adaptive_display_threshold renders on one device: the window crosses the tiles that several devices would own")
        if self.despike_dual and not self.denoise_dual:  # (after every older rule: each of their texts is still raised first)
            raise ValueError("despike_dual needs denoise_dual: it despikes the two halves")

    def select_candidates(self):
        """The candidates of denoise_dual_select, as render.denoise_dual_select takes them: the unguided filter at denoise_k, and the guided one at k = 1.0
        with denoise_feature_k and denoise_feature_tau."""
        return [dict(k=self.denoise_k, alpha=self.denoise_alpha), dict(k=1.0, alpha=self.denoise_alpha, guided=True, k_f=self.denoise_feature_k,
                                                                      tau=self.denoise_feature_tau, **self.slope_keyword())]

    def nlm_keywords(self):
        """The non-local-means filters' parameters (render.denoise, denoise_guided, denoise_dual) from the settings."""
        return dict(radius=self.denoise_radius, patch_radius=self.denoise_patch, k=self.denoise_k, alpha=self.denoise_alpha)

    def atrous_keywords(self):
        """The a-trous filters' parameters (render.denoise_atrous, denoise_atrous_dual) from the settings."""
        return dict(levels=self.denoise_atrous_levels, k=self.denoise_atrous_k, alpha=self.denoise_alpha)

    def guide_keywords(self, atrous=False):
        """The feature weight's parameters for a guided filter — a non-local-means one, or with `atrous` an a-trous one —: k_f, tau and that family's slope
        keyword.  The feature buffers and their counts are the caller's (render._guide)."""
        return dict(k_f=self.denoise_feature_k, tau=self.denoise_feature_tau, **(self.atrous_slope_keyword() if atrous else self.slope_keyword()))

    def slope_keyword(self):
        """{} while denoise_feature_slope is off — the calls made are then those made before it existed —, else dict(slope=denoise_feature_slope)."""
        return dict(slope=self.denoise_feature_slope) if self.denoise_feature_slope > 0.0 else {}

    def atrous_slope_keyword(self):
        """{} while denoise_atrous_slope is off — the calls made are then those made before it existed —, else dict(slope=denoise_atrous_slope)."""
        return dict(slope=self.denoise_atrous_slope) if self.denoise_atrous_slope > 0.0 else {}

    def check_adaptive(self):
        """Raises ValueError for adaptive settings render_tiled cannot follow."""
        if not self.adaptive_threshold >= 0.0:
            raise ValueError("adaptive_threshold must be >= 0 (0 = off)")
        if self.adaptive_threshold > 0.0 and self.samples_per_iteration == 0:
            raise ValueError("adaptive_threshold > 0 needs samples_per_iteration > 0 (the error is checked between passes)")
        if not (self.adaptive_floor > 0.0 and np.isfinite(self.adaptive_floor)):
            raise ValueError("adaptive_floor must be finite and > 0")
        if not (isinstance(self.adaptive_measure, str) and self.adaptive_measure in abi.ADAPTIVE_MEASURES):
            raise ValueError('adaptive_measure must be "channel_max", "luma_tile" or "luma_pixel"')
        if not (self.adaptive_display_threshold >= 0.0 and np.isfinite(self.adaptive_display_threshold)):
            raise ValueError("adaptive_display_threshold must be finite and >= 0 (0 = off)")
        if self.adaptive_display_threshold > 0.0 and self.samples_per_iteration == 0:
            raise ValueError("adaptive_display_threshold > 0 needs samples_per_iteration > 0 (the error is checked between passes)")
        if self.adaptive_display_threshold > 0.0 and self.adaptive_threshold > 0.0:
            raise ValueError("adaptive_display_threshold and adaptive_threshold are mutually exclusive")
        if self.adaptive_display_threshold > 0.0 and self.adaptive_measure != "channel_max":
            raise ValueError("adaptive_display_threshold cannot be combined with adaptive_measure: the display rule is a measure of its own")
        if not (self.adaptive_display_exposure > 0.0 and np.isfinite(self.adaptive_display_exposure)):
            raise ValueError("adaptive_display_exposure must be finite and > 0")
        if not (self.adaptive_display_gamma > 0.0 and np.isfinite(self.adaptive_display_gamma)):
            raise ValueError("adaptive_display_gamma must be finite and > 0")
        if not 0.0 < self.adaptive_display_floor < 1.0:
            raise ValueError("adaptive_display_floor must be finite and in (0, 1)")

    def check_denoise(self):
        """Raises ValueError for denoise settings rmd_denoise / rmd_denoise_guided refuse (checked whether or not denoise is on)."""
        for name, hi in (("denoise_radius", 12), ("denoise_patch", 4)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= hi:
                raise ValueError("%s must be an integer in [0, %d]" % (name, hi))
        if not (self.denoise_k > 0.0 and np.isfinite(self.denoise_k)):
            raise ValueError("denoise_k must be finite and > 0")
        if not (self.denoise_alpha >= 0.0 and np.isfinite(self.denoise_alpha)):
            raise ValueError("denoise_alpha must be finite and >= 0")
        if not (self.denoise_feature_k > 0.0 and np.isfinite(self.denoise_feature_k)):
            raise ValueError("denoise_feature_k must be finite and > 0")
        if not (self.denoise_feature_tau > 0.0 and np.isfinite(self.denoise_feature_tau)):
            raise ValueError("denoise_feature_tau must be finite and > 0")
        if not (self.denoise_feature_slope >= 0.0 and np.isfinite(self.denoise_feature_slope)):
            raise ValueError("denoise_feature_slope must be finite and >= 0 (0 = off)")
        if self.denoise_feature_slope > 0.0 and (self.denoise_atrous or self.denoise_dual_atrous):
            raise ValueError("denoise_feature_slope cannot be combined with denoise_atrous / denoise_dual_atrous: the a-trous filters have no slope term")
        if self.denoise_feature_slope > 0.0 and not (self.denoise_features or self.denoise_dual_features or self.denoise_dual_select):
            raise ValueError("denoise_feature_slope > 0 needs a guided non-local-means filter (denoise_features, denoise_dual_features or denoise_dual_select)")
        if not (self.denoise_atrous_slope >= 0.0 and np.isfinite(self.denoise_atrous_slope)):
            raise ValueError("denoise_atrous_slope must be finite and >= 0 (0 = off)")
        if self.denoise_atrous_slope > 0.0 and not ((self.denoise_atrous and self.denoise_features) or (self.denoise_dual_atrous and self.denoise_dual_features)):
            raise ValueError("denoise_atrous_slope > 0 needs a guided a-trous filter (denoise_atrous with denoise_features, or denoise_dual_atrous with "
                             "denoise_dual_features)")
        v = self.denoise_atrous_levels
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= abi.RMD_ATROUS_MAX_LEVELS:
            raise ValueError("denoise_atrous_levels must be an integer in [0, %d]" % abi.RMD_ATROUS_MAX_LEVELS)
        if not (self.denoise_atrous_k > 0.0 and np.isfinite(self.denoise_atrous_k)):
            raise ValueError("denoise_atrous_k must be finite and > 0")
        if self.denoise_atrous and not self.denoise:
            raise ValueError("denoise_atrous needs denoise")
        if self.denoise_atrous and self.denoise_dual:
            raise ValueError("denoise_atrous cannot be combined with denoise_dual: rmd_denoise_atrous has no dual form")
        if self.denoise_features and not self.denoise:
            raise ValueError("denoise_features needs denoise")
        if self.denoise_dual and not self.denoise:
            raise ValueError("denoise_dual needs denoise")
        if self.denoise_dual and self.samples_per_iteration == 0:
            raise ValueError("denoise_dual needs samples_per_iteration > 0 (the passes alternate between the two half buffers)")
        if self.denoise_dual and self.denoise_features:
            raise ValueError("denoise_dual cannot be combined with denoise_features: rmd_denoise_dual has no feature weight")
        if self.denoise_dual_features and not self.denoise_dual:
            raise ValueError("denoise_dual_features needs denoise_dual (it selects rmd_denoise_dual_guided)")
        if self.denoise_dual_select and not self.denoise_dual:
            raise ValueError("denoise_dual_select needs denoise_dual (it selects rmd_denoise_dual_select)")
        if self.denoise_dual_atrous and not self.denoise_dual:
            raise ValueError("denoise_dual_atrous needs denoise_dual (it selects rmd_denoise_atrous_dual)")
        if self.denoise_dual_atrous and self.denoise_dual_select:
            raise ValueError("denoise_dual_atrous cannot be combined with denoise_dual_select: the selection has no a-trous candidate")
        if self.denoise_dual_atrous_region and not self.denoise_dual_atrous:
            raise ValueError("denoise_dual_atrous_region needs denoise_dual_atrous (it selects rmd_denoise_atrous_dual_region for the adaptive check)")
        if not self.adaptive_denoised_threshold >= 0.0:
            raise ValueError("adaptive_denoised_threshold must be >= 0 (0 = off)")
        if self.adaptive_denoised_threshold > 0.0 and not self.denoise_dual:
            raise ValueError("adaptive_denoised_threshold > 0 needs denoise_dual (the error is that of the dual-buffer filter)")
        if self.adaptive_denoised_threshold > 0.0 and self.adaptive_threshold > 0.0:
            raise ValueError("adaptive_denoised_threshold and adaptive_threshold are mutually exclusive")
        v = self.adaptive_min_samples
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("adaptive_min_samples must be an integer >= 0")
        if self.denoise_dual and self.adaptive_measure != "channel_max":
            raise ValueError("adaptive_measure cannot be combined with denoise_dual: the dual loop's check is rmd_tile_error_dual")
        if self.denoise_dual and self.adaptive_display_threshold > 0.0:
            raise ValueError("adaptive_display_threshold cannot be combined with denoise_dual: the dual loop's check is rmd_tile_error_dual")
        if not (self.adaptive_denoised_display_threshold >= 0.0 and np.isfinite(self.adaptive_denoised_display_threshold)):
            raise ValueError("adaptive_denoised_display_threshold must be finite and >= 0 (0 = off)")
        if self.adaptive_denoised_display_threshold > 0.0 and self.samples_per_iteration == 0:
            raise ValueError("adaptive_denoised_display_threshold > 0 needs samples_per_iteration > 0 (the error is checked between passes)")
        if self.adaptive_denoised_display_threshold > 0.0 and not self.denoise_dual:
            raise ValueError("adaptive_denoised_display_threshold > 0 needs denoise_dual (the error is that of the dual-buffer filter)")
        if self.adaptive_denoised_display_threshold > 0.0 and self.adaptive_denoised_threshold > 0.0:
            raise ValueError("adaptive_denoised_display_threshold and adaptive_denoised_threshold are mutually exclusive")
        if self.adaptive_denoised_display_threshold > 0.0 and self.adaptive_threshold > 0.0:
            raise ValueError("adaptive_denoised_display_threshold and adaptive_threshold are mutually exclusive")

    def check_preview(self, n_devices=1):
        """Raises ValueError for preview settings render_tiled cannot follow on `n_devices` devices."""
        v = self.preview_every
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("preview_every must be an integer >= 0 (0 = off)")
        if self.preview_every > 0 and self.samples_per_iteration == 0:
            raise ValueError("preview_every > 0 needs samples_per_iteration > 0 (a preview is made between passes)")
        if not (self.preview_exposure > 0.0 and np.isfinite(self.preview_exposure)):
            raise ValueError("preview_exposure must be finite and > 0")
        if not (self.preview_gamma > 0.0 and np.isfinite(self.preview_gamma)):
            raise ValueError("preview_gamma must be finite and > 0")
        if self.preview_denoise and self.preview_every == 0:
            raise ValueError("preview_denoise needs preview_every > 0 (it selects the filter of the previews)")
        if self.preview_denoise and n_devices != 1:
            raise ValueError("preview_denoise renders on one device: the filter's window crosses the tiles that several devices would own")
        if self.preview_auto_exposure and self.preview_every == 0:
            raise ValueError("preview_auto_exposure needs preview_every > 0 (it sets the exposure of the previews)")
        if not (0.0 < self.auto_exposure_percentile <= 1.0):  # (rmd_exposure_from_histogram's rules; a NaN fails both)
            raise ValueError("auto_exposure_percentile must be finite and in (0, 1]")
        if not (0.0 < self.auto_exposure_target < 1.0):
            raise ValueError("auto_exposure_target must be finite and in (0, 1)")

    def pod(self, sample_begin=0, sample_count=None):
        s = abi.Settings()
        s.bounce_limit = self.bounce_limit
        s.sample_begin = int(sample_begin)
        s.sample_count = self.sample_count if sample_count is None else int(sample_count)
        s.seed = self.seed
        s.flags = ((abi.RMD_RENDER_DOF if self.use_dof else 0) | (abi.RMD_RENDER_TRACE_BLACK_PATHS if self.trace_black_paths else 0)
                   | (abi.RMD_RENDER_END_BLACK_PATHS if self.end_black_paths else 0))
        return s


def generate_tiles(width, height, tile_size):
    """Tile generation order of render_tiled (src/trace.rs:142-173): column-major, edge tiles clamped."""
    tw, th = tile_size
    tiles = []
    x = y = 0
    while True:
        x1 = min(x + tw, width)
        y1 = min(y + th, height)
        tiles.append((x, y, x1 - x, y1 - y))
        y += th
        if y >= height:
            y = 0
            x += tw
        if x >= width:
            break
    return tiles


def tile_array(tiles):
    arr = (abi.TileRect * max(1, len(tiles)))()
    for i, (l, t, w, h) in enumerate(tiles):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr
