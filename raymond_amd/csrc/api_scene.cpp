// C-ABI implementation (include/raymond_hip.h) of scene upload: what rmd_scene_create derives from the caller's objects and grids on the host, the
// upload, and the scene's end.  Host code only.
#define RMD_WITH_HIP 1
#include "internal.hpp"
#include "launch.hpp"

extern "C" {

// What rmd_scene_create derives from a grid description before it uploads it (device_types.hpp: DevGrid): validated tables, the triangle
// records, the per-cell index lists with their entries, the Heron constants.  ~50 ms of host time for the 99k-triangle benchmark mesh — a host
// scheduler creates a scene per render_tiled call and per GPU (the counterpart of the reference's per-worker `scene.clone()`, src/trace.rs:182-185),
// so a description that comes from a rmd_grid_build (rmd_grid_desc::built) keeps them in that object: derived once, shared by every upload.
struct GridDerived {
	std::vector<unsigned char> recs;
	std::vector<rmd::CellEntry> entries;
	std::vector<uint32_t> ids;
	std::vector<double> aux;
	std::vector<double> spheres; // per triangle: centre and squared radius of a sphere around it, inflated (device_types.hpp: DevGrid::tri_sph)
	double sphere_kb = 0.0;      // ... and the grid's distance-proportional allowance (DevGrid::sph_kb)
};
static rmd_status derive_grid_tables(rmd_context *ctx, const rmd_grid_desc &g, GridDerived &out) {
	{
		if (!g.cells || !g.mapping_table || !g.tri_pos || !g.tri_nrm || g.n_tris == 0 ||
		    g.n_cells != (uint64_t)g.resolution[0] * g.resolution[1] * g.resolution[2]) {
			return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: inconsistent grid description");
		}
		// validate the CSR-like table so that the kernel's gathers stay in bounds
		for (uint64_t c = 0; c < g.n_cells; c++) {
			uint64_t off = g.cells[c];
			if (off >= g.n_mapping || off + (uint64_t)g.mapping_table[off] >= g.n_mapping) {
				return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: cells/mapping_table run out of range");
			}
			uint32_t cnt = g.mapping_table[off];
			for (uint32_t k = 1; k <= cnt; k++)
				if (g.mapping_table[off + k] >= g.n_tris) {
					return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: triangle index out of range in mapping_table");
				}
		}
		// the kernel keeps the reference's linear cell index x + res.x*(y + z*res.z) in 32 bits
		if ((uint64_t)g.resolution[0] * ((uint64_t)g.resolution[1] + (uint64_t)g.resolution[2] * g.resolution[2]) >= (1ull << 31) ||
		    g.n_cells > (1ull << 31)) {
			return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_scene_create: grid resolution too large for 31-bit cell indices");
		}
		// triangle records, per-cell lists of triangle indices and the cell entries (device_types.hpp): record = v0, edge1 = v1 - v0,
		// edge2 = v2 - v0 (triangle.rs:16-17, same subtraction, done once); entry slot 0 = the cell's list in mapping_table order, slots 1..6 =
		// that list without the triangles the cell at index c - delta_s lists too (the cell a walk came from: tested already, missed)
		const uint64_t n_refs = g.n_mapping - g.n_cells;
		if (n_refs > 0xFFFFFFFFull) {
			return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_scene_create: more than 2^32-1 cell->triangle references");
		}
		std::vector<unsigned char> &recs = out.recs;
		recs.assign((size_t)g.n_tris * rmd::kTriRecStride, 0);
		for (uint64_t ti = 0; ti < g.n_tris; ti++) {
			const double *p = g.tri_pos + (size_t)ti * 9;
			double q[9];
			for (int a = 0; a < 3; a++) q[a] = p[a], q[3 + a] = p[3 + a] - p[a], q[6 + a] = p[6 + a] - p[a];
			std::memcpy(recs.data() + (size_t)ti * rmd::kTriRecStride, q, sizeof(q));
		}
		std::vector<rmd::CellEntry> &entries = out.entries;
		entries.assign((size_t)g.n_cells * rmd::kEntrySlots, rmd::CellEntry{0u, 0u});
		std::vector<uint32_t> &ids = out.ids;
		ids.clear();
		ids.reserve((size_t)n_refs * 3);
		{
			uint64_t refs_seen = 0;
			for (uint64_t c = 0; c < g.n_cells; c++) { // slot 0: the full lists, validated against overlapping runs
				const uint32_t off = g.cells[c], cnt = g.mapping_table[off];
				refs_seen += cnt;
				if (refs_seen > n_refs) { // cells sharing a run: the tables are not the builder's; refuse rather than overflow
							return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: cells/mapping_table runs overlap");
				}
				entries[c * rmd::kEntrySlots] = rmd::CellEntry{(uint32_t)ids.size(), cnt};
				ids.insert(ids.end(), g.mapping_table + off + 1, g.mapping_table + off + 1 + cnt);
			}
			const int64_t sx = (int64_t)g.resolution[0], sxz = (int64_t)g.resolution[0] * (int64_t)g.resolution[2]; // Q5: res.z where res.y is meant
			const int64_t delta[7] = {0, 1, -1, sx, -sx, sxz, -sxz};
			std::vector<uint32_t> fresh;
			std::vector<uint64_t> listed_by((size_t)g.n_tris, ~0ull); // triangle -> the (cell, slot) pass that last saw it in a predecessor's list
			for (uint64_t c = 0; c < g.n_cells; c++) {
				const rmd::CellEntry full = entries[c * rmd::kEntrySlots];
				const uint32_t *mine = g.mapping_table + g.cells[c] + 1;
				for (uint32_t s = 1; s < rmd::kEntrySlots; s++) {
					rmd::CellEntry &e = entries[c * rmd::kEntrySlots + s];
					e = full;
					if (s == 7u || full.count == 0u) continue;
					const int64_t prev = (int64_t)c - delta[s];
					if (prev < 0 || prev >= (int64_t)g.n_cells || prev == (int64_t)c) continue; // no such predecessor: never asked for
					const uint32_t poff = g.cells[prev], pcnt = g.mapping_table[poff];
					if (pcnt == 0u) continue;
					const uint32_t *theirs = g.mapping_table + poff + 1;
					fresh.clear();
					const uint64_t pass = c * rmd::kEntrySlots + s;
					for (uint32_t j = 0; j < pcnt; j++) listed_by[theirs[j]] = pass;
					for (uint32_t k = 0; k < full.count; k++)
						if (listed_by[mine[k]] != pass) fresh.push_back(mine[k]);
					if (fresh.size() == full.count) continue; // nothing to leave out: shares the full list
					e = rmd::CellEntry{(uint32_t)ids.size(), (uint32_t)fresh.size()};
					ids.insert(ids.end(), fresh.begin(), fresh.end());
					if (ids.size() > 0xFFFFFFFFull) {
									return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_scene_create: triangle index lists exceed 2^32 entries");
					}
				}
			}
		}
		out.aux.assign((size_t)g.n_tris * 4, 0.0);
		for (uint64_t ti = 0; ti < g.n_tris; ti++) rmd::triangle_aux(g.tri_pos + (size_t)ti * 9, out.aux.data() + (size_t)ti * 4);
		out.spheres.assign((size_t)g.n_tris * 4, 0.0);
		out.sphere_kb = 0.0;
		for (uint64_t ti = 0; ti < g.n_tris; ti++) {
			double kb = 0.0;
			rmd::triangle_sphere(g.tri_pos + (size_t)ti * 9, out.spheres.data() + (size_t)ti * 4, kb);
			out.sphere_kb = std::max(out.sphere_kb, kb);
		}
	}
	return RMD_OK;
}

// What rmd_scene_create derives from the caller's objects on the host, before anything is uploaded: the device records, whether the scene's
// parameters are regular, the pairs of opposite planes, the axis rule's walls and the object loops' turns.  A function of its own because the
// host-only probe rmd_probe_primary_candidates (probe.cpp) needs exactly what a scene would hold, without a device.
extern "C++" rmd_status rmd::derive_scene_objects(rmd_context *ctx, const rmd_object *objects, uint32_t n_objects, uint32_t n_grids, int64_t axis_pairs_tunable, rmd::SceneObjects &out) {
	std::vector<rmd::DevObject> &hobj = out.objs;
	hobj.assign(n_objects, rmd::DevObject{});
	bool regular = true;
	for (uint32_t i = 0; i < n_objects; i++) {
		const rmd_object &o = objects[i];
		rmd::DevObject &d = hobj[i];
		std::memset(&d, 0, sizeof(d));
		if (o.geometry_kind > RMD_GEOM_GRID) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: unknown geometry kind");
		if (o.material.kind > RMD_MAT_EMISSION) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: unknown material kind");
		if (o.geometry_kind == RMD_GEOM_GRID && o.grid_index >= n_grids) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: grid_index out of range");
		d.geometry_kind = o.geometry_kind, d.grid_index = o.grid_index, d.material_kind = o.material.kind;
		for (int a = 0; a < 3; a++) d.origin[a] = o.origin[a], d.normal[a] = o.normal[a], d.color[a] = o.material.color[a];
		d.radius = o.radius;
		// the GGX angle roughness^2 * sqrt(u / (1 - u)) must stay inside sincos_cw's reduction range (device_core.hpp)
		if (o.material.kind != RMD_MAT_EMISSION && std::fabs(o.material.roughness) > rmd::kMaxRoughness)
			return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_scene_create: |roughness| > 512 is not supported");
		// (the bounce weight is formed as ONE quotient whose denominator holds (roughness^2 / 8)^2 for a surface seen from behind: it must not underflow)
		if (o.material.kind != RMD_MAT_EMISSION && o.material.roughness != 0.0 && std::fabs(o.material.roughness) < rmd::kMinRoughness)
			return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_scene_create: 0 < |roughness| < 1e-12 is not supported");
		d.roughness = o.material.roughness;
		d.metalness = o.material.kind == RMD_MAT_METAL ? 1.0 : 0.0; // src/trace.rs:248-249
		// Is this object inside the class of parameters for which "a path whose throughput is exactly (0, 0, 0) contributes exactly (0, 0, 0)" is
		// proved?  The proof needs every later vertex of such a path to have a FINITE radiance (0 x NaN = NaN, src/trace.rs:
		// 281-282, :315-318).  Outside the class — an Emission of (inf, 0, 0), a NaN or infinite colour / position / normal, coordinates so large that a
		// hit point overflows, a sphere of radius 0 (normalize(P - centre) of a hit at the centre), a material of roughness 0 (geometry_schlick_ggx is
		// 0 / 0 for a surface seen from behind, :372-378) — the reference's sample can be NaN without any mesh, so flags 0 traces such a scene's
		// black paths on, as it does a scene with a grid (make_params).
		{
			auto tame = [](double v) { return std::fabs(v) <= 1e150; }; // finite, and no sum or product of two of them overflows
			bool ok = true;
			if (o.geometry_kind != RMD_GEOM_GRID)
				for (int a = 0; a < 3; a++) ok = ok && tame(o.origin[a]);
			if (o.geometry_kind == RMD_GEOM_PLANE)
				for (int a = 0; a < 3; a++) ok = ok && tame(o.normal[a]);
			if (o.geometry_kind == RMD_GEOM_SPHERE) ok = ok && tame(o.radius) && o.radius != 0.0 && o.radius * o.radius > 0.0;
			for (int a = 0; a < 3; a++) ok = ok && tame(o.material.color[a]);
			if (o.material.kind != RMD_MAT_EMISSION) ok = ok && tame(o.material.roughness) && o.material.roughness != 0.0;
			regular = regular && ok;
		}
		if (o.material.kind == RMD_MAT_DIFFUSE && o.material.color[0] == 0.0 && o.material.color[1] == 0.0 && o.material.color[2] == 0.0) d.flags |= rmd::kObjBlackDiffuse;
	}
	// pair_opposite_planes: plane j is tested together with the first earlier, still unpaired plane i whose normal is its exact negation
	// (device_core.hpp: plane_pair_intersect — the facing conditions of such planes exclude each other, one division serves both)
	for (uint32_t j = 0; j < n_objects; j++) {
		if (hobj[j].geometry_kind != RMD_GEOM_PLANE) continue;
		for (uint32_t i = 0; i < j; i++) {
			if (hobj[i].geometry_kind != RMD_GEOM_PLANE || hobj[i].pair_info != 0u) continue;
			bool opposite = true; // NaN components compare unequal: never paired
			for (int a = 0; a < 3; a++) opposite = opposite && hobj[j].normal[a] == -hobj[i].normal[a];
			if (!opposite) continue;
			hobj[i].pair_info = rmd::kPairTestedAtPartner | j, hobj[j].pair_info = i + 1u;
			break;
		}
	}
	// ... and a pair whose normals are exactly +e_k and -e_k — the walls of an axis-aligned room — is tested with one component of the ray instead of
	// three dot products (scene_split.hpp: axis_pairs_visit has the argument for "same bits"): one pair per axis, in scenes of regular parameters
	uint32_t axis_pairs = 0;
	for (uint32_t j = 0; j < n_objects && j < 1023u && regular && axis_pairs_tunable != 1; j++) {
		if (hobj[j].geometry_kind != RMD_GEOM_PLANE || hobj[j].pair_info == 0u || (hobj[j].pair_info & rmd::kPairTestedAtPartner)) continue;
		const uint32_t i = hobj[j].pair_info - 1u;
		int k = -1, nonzero = 0;
		for (int a = 0; a < 3; a++)
			if (hobj[i].normal[a] != 0.0) nonzero++, k = a;
		if (nonzero != 1 || (hobj[i].normal[k] != 1.0 && hobj[i].normal[k] != -1.0) || ((axis_pairs >> (10 * k)) & 1023u) != 0u) continue;
		axis_pairs |= (j + 1u) << (10 * k);
		hobj[j].flags |= rmd::kObjAxisPair | ((uint32_t)k << rmd::kObjAxisShift) | (hobj[i].normal[k] == 1.0 ? rmd::kObjAxisEarlierIsPlus : 0u);
		hobj[i].flags |= rmd::kObjAxisPair;
		hobj[j].partner_origin_k = hobj[i].origin[k];
		hobj[j].pair_info = rmd::kPairTestedAtPartner | rmd::kPairAxis | i; // the object loops pass both planes by ("tested at its partner's turn"):
		hobj[i].pair_info |= rmd::kPairAxis;                                 // their turn is axis_pairs_visit's, ahead of the loop
	}
	// the axis pairs as the axis rule reads them (device_types.hpp: AxisWalls)
	{
		rmd::AxisWalls *walls = out.walls;
		std::memset(walls, 0, 3 * sizeof(rmd::AxisWalls));
		for (int k = 0; k < 3; k++) {
			const uint32_t f = (axis_pairs >> (10 * k)) & 1023u;
			if (f == 0u) continue;
			const uint32_t j = f - 1u, i = hobj[j].pair_info & 0x3FFFFFFFu; // the later and the earlier plane of the pair
			const bool e_plus = (hobj[j].flags & rmd::kObjAxisEarlierIsPlus) != 0u;
			walls[k].o_plus = e_plus ? hobj[i].origin[k] : hobj[j].origin[k], walls[k].o_minus = e_plus ? hobj[j].origin[k] : hobj[i].origin[k];
			walls[k].idx_plus = e_plus ? i : j, walls[k].idx_minus = e_plus ? j : i;
		}
	}
	// the object loops' turns (device_types.hpp: RenderParams::visit_mask): a plane tested at its partner's turn or by the axis rule has none
	out.visit_mask = 0ull, out.grid_mask = 0ull;
	for (uint32_t i = 0; i < n_objects && i < 64u; i++) {
		if (!(hobj[i].geometry_kind == RMD_GEOM_PLANE && (hobj[i].pair_info & rmd::kPairTestedAtPartner))) out.visit_mask |= 1ull << i;
		if (hobj[i].geometry_kind == RMD_GEOM_GRID) out.grid_mask |= 1ull << i;
	}
	out.regular = regular, out.axis_pairs = axis_pairs;
	return RMD_OK;
}

static rmd_status scene_create_impl(rmd_context *ctx, const rmd_object *objects, uint32_t n_objects, const rmd_grid_desc *grids, uint32_t n_grids,
                                    rmd_scene **out) {
	if (rmd_status s = rmd::bind(ctx)) return s;
	if (!out || (n_objects && !objects) || (n_grids && !grids)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_scene_create: null argument");
	rmd::SceneObjects derived;
	if (rmd_status s = rmd::derive_scene_objects(ctx, objects, n_objects, n_grids, ctx->tunable[RMD_TUNE_AXIS_PAIRS], derived)) return s;
	std::vector<rmd::DevObject> &hobj = derived.objs;
	const bool regular = derived.regular;
	const uint32_t axis_pairs = derived.axis_pairs;
	// (the scene under construction: an early return or an exception — std::bad_alloc from one of the host-side tables: a 256^3 grid needs a
	// gigabyte for its cell entries alone — releases what has been uploaded)
	auto sc = std::make_unique<rmd_scene>();
	sc->ctx = ctx, sc->n_objects = n_objects, sc->n_grids = n_grids, sc->regular = regular;
	sc->axis_pairs = axis_pairs;
	// the axis pairs as the axis rule reads them, behind the table's last record (device_types.hpp: AxisWalls)
	rmd::DevObject walls_block;
	std::memset(&walls_block, 0, sizeof(walls_block));
	std::memcpy(&walls_block, derived.walls, sizeof(derived.walls));
	sc->visit_mask = derived.visit_mask, sc->grid_mask = derived.grid_mask;
	for (uint32_t i = 0; i < n_objects; i++)
		if (objects[i].geometry_kind == RMD_GEOM_PLANE) sc->planes.insert(sc->planes.end(), objects[i].origin, objects[i].origin + 3), sc->planes.insert(sc->planes.end(), objects[i].normal, objects[i].normal + 3);
	// the generation trips' own candidate sets and the items' tile classes (primary_candidates.hpp): a regular scene without a grid, unless
	// RMD_TUNE_AXIS_PAIRS says 1 or 2 (neither) or 3 (no tile classes)
	sc->primary_cull = rmd::primary_cull_bits(regular, n_grids, ctx->tunable[RMD_TUNE_AXIS_PAIRS]);
	for (uint32_t i = 0; i < n_objects; i++) sc->n_grid_objects += objects[i].geometry_kind == RMD_GEOM_GRID ? 1u : 0u;
	auto upload = [&](const void *src, size_t bytes, void **dst) -> hipError_t {
		*dst = nullptr;
		rmd::DeviceBuffer b;
		hipError_t e = b.alloc(bytes ? bytes : 16);
		if (e != hipSuccess) return e;
		*dst = b.as<void>();
		sc->owned.push_back(std::move(b));
		if (bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
		return e;
	};
	std::vector<rmd::DevGrid> hgrid(n_grids);
	for (uint32_t gi = 0; gi < n_grids; gi++) {
		const rmd_grid_desc &g = grids[gi];
		rmd::DevGrid &d = hgrid[gi];
		std::memset(&d, 0, sizeof(d));
		// the derived tables: from the rmd_grid_build this description came from (derived once, kept there), or made here
		std::shared_ptr<const GridDerived> derived;
		{
			rmd_grid_build *gb = const_cast<rmd_grid_build *>(g.built);
			const bool from_build = gb && gb->cells.data() == g.cells && gb->cells.size() == g.n_cells && gb->mapping.data() == g.mapping_table &&
			                        gb->mapping.size() == g.n_mapping && gb->pos.data() == g.tri_pos && gb->nrm.data() == g.tri_nrm && gb->pos.size() == g.n_tris * 9;
			std::unique_lock<std::mutex> lock;
			if (from_build) {
				lock = std::unique_lock<std::mutex>(gb->derived_mutex);
				derived = std::static_pointer_cast<const GridDerived>(gb->derived);
			}
			if (!derived) {
				auto fresh = std::make_shared<GridDerived>();
				if (rmd_status st = derive_grid_tables(ctx, g, *fresh)) return st;
				derived = fresh;
				if (from_build) gb->derived = fresh;
			}
		}
		const std::vector<unsigned char> &recs = derived->recs;
		const std::vector<rmd::CellEntry> &entries = derived->entries;
		const std::vector<uint32_t> &ids = derived->ids;
		const std::vector<double> &aux = derived->aux;
		for (int a = 0; a < 3; a++) {
			d.bbox_min[a] = g.bbox_min[a], d.bbox_max[a] = g.bbox_max[a], d.cell_size[a] = g.cell_size[a];
			d.inv_cell_size[a] = rmd::exact_reciprocal(g.cell_size[a]);
			d.res[a] = g.resolution[a];
			if (a == 2) sc->walk_steps_bound = std::max<uint32_t>(sc->walk_steps_bound, (uint32_t)std::min<uint64_t>((uint64_t)g.resolution[0] + g.resolution[1] + g.resolution[2] + 3u, 0xFFFFFFFFull));
		}
		d.n_cells = g.n_cells, d.n_tris = g.n_tris;
		uint64_t last_nonempty = 0;
		bool any_nonempty = false;
		for (uint64_t c = 0; c < g.n_cells; c++)
			if (entries[c * rmd::kEntrySlots].count) last_nonempty = c, any_nonempty = true;
		// occupancy bitmask for LDS: bit i covers cells [i << shift, (i+1) << shift); only up to the last non-empty cell
		// the mask covers every cell of the array when that fits the budget (the stepping loop's lean form then needs no clamp of the index),
		// else the cells up to the last non-empty one (indices past it read the all-zero word that ends every mask)
		uint64_t covered = any_nonempty ? last_nonempty + 1 : 0;
		size_t budget_bytes = rmd::kMaskBudgetBytes;
		if (ctx->tunable[RMD_TUNE_MASK_BUDGET] > 0) budget_bytes = (size_t)ctx->tunable[RMD_TUNE_MASK_BUDGET]; // forces coarser masks
		if (budget_bytes < 64) budget_bytes = 64;
		if (budget_bytes > rmd::kMaskBudgetBytes) budget_bytes = rmd::kMaskBudgetBytes;
		const size_t budget_words = budget_bytes / 4 / n_grids;
		if (budget_words < 2) // one data word + the all-zero pad word is the smallest mask
			return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_scene_create: too many grids for the LDS occupancy-mask budget");
		if ((g.n_cells + 31) / 32 + 1 <= budget_words) covered = g.n_cells;
		uint32_t shift = 0;
		while (shift < 63 && ((covered >> shift) + 31) / 32 + 1 > budget_words) shift++;
		const uint64_t bits = covered ? ((covered - 1) >> shift) + 1 : 0;
		std::vector<uint32_t> mask((size_t)((bits + 31) / 32) + 1, 0u); // + one all-zero word: indices past the mask read it
		for (uint64_t c = 0; c < covered; c++)
			if (entries[c * rmd::kEntrySlots].count) mask[(c >> shift) >> 5] |= 1u << ((c >> shift) & 31u);
		d.mask_bits = (uint32_t)bits, d.mask_shift = shift, d.mask_n_words = (uint32_t)mask.size();
		d.mask_lds_word = sc->mask_words_total;
		sc->mask_words_total += (uint32_t)((mask.size() + 3) & ~(size_t)3);
		void *p = nullptr;
		RMD_HIP(ctx, upload(entries.data(), entries.size() * sizeof(rmd::CellEntry), &p));
		d.cell_entries = (const rmd::CellEntry *)p;
		RMD_HIP(ctx, upload(ids.data(), ids.size() * sizeof(uint32_t), &p));
		d.tri_ids = (const uint32_t *)p;
		RMD_HIP(ctx, upload(recs.data(), recs.size(), &p));
		d.tri_recs = p;
		RMD_HIP(ctx, upload(mask.data(), mask.size() * sizeof(uint32_t), &p));
		d.mask_words = (const uint32_t *)p;
		RMD_HIP(ctx, upload(g.tri_pos, g.n_tris * 9 * sizeof(double), &p));
		d.tri_pos = (const double *)p;
		RMD_HIP(ctx, upload(g.tri_nrm, g.n_tris * 9 * sizeof(double), &p));
		d.tri_nrm = (const double *)p;
		RMD_HIP(ctx, upload(aux.data(), aux.size() * sizeof(double), &p));
		d.tri_aux = (const double *)p;
		RMD_HIP(ctx, upload(derived->spheres.data(), derived->spheres.size() * sizeof(double), &p));
		d.tri_sph = (const double *)p, d.sph_kb = derived->sphere_kb;
	}
	void *p = nullptr;
	hobj.push_back(walls_block); // (uploaded behind the table; n_objects does not count it)
	RMD_HIP(ctx, upload(hobj.data(), hobj.size() * sizeof(rmd::DevObject), &p));
	sc->d_objects = (rmd::DevObject *)p;
	RMD_HIP(ctx, upload(hgrid.data(), hgrid.size() * sizeof(rmd::DevGrid), &p));
	sc->d_grids = (rmd::DevGrid *)p;
	*out = sc.release();
	return RMD_OK;
}

rmd_status rmd_scene_create(rmd_context *ctx, const rmd_object *objects, uint32_t n_objects, const rmd_grid_desc *grids, uint32_t n_grids,
                            rmd_scene **out) {
	if (out) *out = nullptr;
	return rmd::guarded(ctx, "rmd_scene_create", [&] { return scene_create_impl(ctx, objects, n_objects, grids, n_grids, out); });
}

// (the launches that read the scene's tables are waited for in the body; `owned` is freed after it)
rmd_scene::~rmd_scene() {
	if (ctx) {
		(void)hipSetDevice(ctx->device);
		(void)hipStreamSynchronize(ctx->stream);
	}
}

void rmd_scene_destroy(rmd_scene *scene) { delete scene; }

} // extern "C"
