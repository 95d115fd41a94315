// GPU-side AccGrid::build_from_mesh (reference core/src/geometry/acc_grid.rs:36-83) — SURVEY.md section 8f row N4.
// Produces the same bounds, cell size and cells / mapping_table bytes as the host builder (grid_build.cpp) and the oracle
// (tests/test_gpu_grid_build.py, on the adversarial meshes of tests/grid_meshes.py):
//   1. host            Mesh::find_mesh_bounds (mesh.rs:123-140): rmd::mesh_bounds (internal.hpp), the fold the host builder uses, in vertex order.
//                      On the host, not a device reduction (there was one, bounds_kernel): a tree of v_min_f64 / v_max_f64 gives the value of
//                      a bound in any order but not the SIGN OF A ZERO bound — it ordered -0.0 < +0.0 where the project's rule is "the later
//                      vertex wins" — and an O(n) fold over an array the host already holds needs no kernel.
//   2. host            estimate_grid_resolution + cell_size (acc_grid.rs:6-17, :38) with the host libm pow, exactly as
//                      grid_build.cpp does, so the truncations agree.
//   3. count_kernel    per triangle: its cell range (:43-56) and one atomicAdd per overlapped cell.
//   4. scan            cells[c] = sum over c' < c of (1 + count[c'])  (:67-74), three-phase device scan.
//   5. fill_kernel     per triangle: claim a slot in each overlapped cell's run with an atomic cursor.
//   6. sort_kernel     per cell: sort its run ascending — the reference pushes indices while iterating the triangles in
//                      order (:42,:61), so every run is ascending; the atomics above fill it in arbitrary order.  An insertion sort in one
//                      lane, quadratic in the run's length: fine for the dozens of entries of a mesh's cells, some 10^8 dependent memory steps for one of 10^4
//                      (the tests keep to runs of at most 1024).
#define RMD_WITH_HIP 1
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "internal.hpp"


namespace {

__constant__ double kSeedMinDev[3] = {125125.0, 1251251.0, 12512512.0};
__constant__ double kSeedMaxDev[3] = {-123125.0, -125123.0, -512123.0};

struct GridDims {
	double bmin[3], cell[3];
	unsigned long long res[3], n_cells;
};

// triangle.rs:70-84 + acc_grid.rs:43-56: cell range of one triangle; false where the reference's usize cast fails
__device__ bool tri_range(const double *p9, const GridDims &g, unsigned lo[3], unsigned hi[3]) {
	for (int a = 0; a < 3; a++) {
		double mn = fmin(fmin(fmin(kSeedMinDev[a], p9[a]), p9[3 + a]), p9[6 + a]);
		double mx = fmax(fmax(fmax(kSeedMaxDev[a], p9[a]), p9[3 + a]), p9[6 + a]);
		double l = (mn - g.bmin[a]) / g.cell[a], h = (mx - g.bmin[a]) / g.cell[a];
		if (!(l > -1.0 && l < 18446744073709551616.0) || !(h > -1.0 && h < 18446744073709551616.0)) return false;
		unsigned long long ul = (unsigned long long)l, uh = (unsigned long long)h;
		lo[a] = (unsigned)(ul < g.res[a] - 1 ? ul : g.res[a] - 1);
		hi[a] = (unsigned)(uh < g.res[a] - 1 ? uh : g.res[a] - 1);
	}
	return true;
}

// mode 0: count[idx]++ ; mode 1: mapping[cells[idx] + 1 + cursor[idx]++] = triangle
__global__ __launch_bounds__(256) void scatter_kernel(int mode, const double *__restrict__ pos, unsigned long long n_tris, GridDims g,
                                                      unsigned *__restrict__ count, const unsigned *__restrict__ cells,
                                                      unsigned *__restrict__ mapping, int *__restrict__ error) {
	unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_tris) return;
	unsigned lo[3], hi[3];
	if (!tri_range(pos + i * 9, g, lo, hi)) {
		atomicExch(error, 1); // "Failed to cast cell bounds to usize" (acc_grid.rs:44-51)
		return;
	}
	for (unsigned long long z = lo[2]; z <= hi[2]; z++)
		for (unsigned long long y = lo[1]; y <= hi[1]; y++)
			for (unsigned long long x = lo[0]; x <= hi[0]; x++) {
				unsigned long long idx = x + g.res[0] * (y + z * g.res[2]); // :61 — res.z where res.y is meant (Q5)
				if (idx >= g.n_cells) {
					atomicExch(error, 2); // the reference panics: index out of bounds
					return;
				}
				unsigned slot = atomicAdd(&count[idx], 1u);
				if (mode == 1) mapping[cells[idx] + 1u + slot] = (unsigned)i;
			}
}

// three-phase exclusive scan of (count[c] + 1) in blocks of 1024 elements (256 threads x 4)
__global__ __launch_bounds__(256) void scan_block_sums(const unsigned *__restrict__ count, unsigned long long n, unsigned long long *__restrict__ block_sums) {
	__shared__ unsigned long long red[256];
	unsigned long long base = (unsigned long long)blockIdx.x * 1024, sum = 0;
	for (int k = 0; k < 4; k++) {
		unsigned long long i = base + threadIdx.x * 4 + k;
		if (i < n) sum += (unsigned long long)count[i] + 1ull;
	}
	red[threadIdx.x] = sum;
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
		__syncthreads();
	}
	if (threadIdx.x == 0) block_sums[blockIdx.x] = red[0];
}
__global__ void scan_of_sums(unsigned long long *block_sums, unsigned n_blocks, unsigned long long *total) { // one thread: n_blocks is small
	unsigned long long run = 0;
	for (unsigned b = 0; b < n_blocks; b++) {
		unsigned long long v = block_sums[b];
		block_sums[b] = run;
		run += v;
	}
	*total = run;
}
__global__ __launch_bounds__(256) void scan_write(const unsigned *__restrict__ count, unsigned long long n, const unsigned long long *__restrict__ block_sums,
                                                  unsigned *__restrict__ cells, unsigned *__restrict__ mapping) {
	__shared__ unsigned long long pre[256];
	unsigned long long base = (unsigned long long)blockIdx.x * 1024, v[4], sum = 0;
	for (int k = 0; k < 4; k++) {
		unsigned long long i = base + threadIdx.x * 4 + k;
		v[k] = i < n ? (unsigned long long)count[i] + 1ull : 0ull;
		sum += v[k];
	}
	pre[threadIdx.x] = sum;
	__syncthreads();
	// Hillis-Steele inclusive scan over the 256 thread sums
	for (int d = 1; d < 256; d <<= 1) {
		unsigned long long add = (int)threadIdx.x >= d ? pre[threadIdx.x - d] : 0ull;
		__syncthreads();
		pre[threadIdx.x] += add;
		__syncthreads();
	}
	unsigned long long run = block_sums[blockIdx.x] + pre[threadIdx.x] - sum;
	for (int k = 0; k < 4; k++) {
		unsigned long long i = base + threadIdx.x * 4 + k;
		if (i < n) {
			cells[i] = (unsigned)run;       // acc_grid.rs:69
			mapping[run] = count[i];        // :70
			run += v[k];
		}
	}
}

__global__ __launch_bounds__(256) void sort_kernel(const unsigned *__restrict__ cells, unsigned long long n_cells, unsigned *__restrict__ mapping) {
	unsigned long long c = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
	if (c >= n_cells) return;
	unsigned off = cells[c], n = mapping[off];
	unsigned *run = mapping + off + 1;
	for (unsigned i = 1; i < n; i++) { // insertion sort: runs hold a handful to a few dozen indices
		unsigned key = run[i], j = i;
		while (j > 0 && run[j - 1] > key) {
			run[j] = run[j - 1];
			j--;
		}
		run[j] = key;
	}
}

} // namespace

static rmd_status grid_build_from_mesh_gpu_impl(rmd_context *ctx, const double *tri_pos, const double *tri_nrm, uint64_t n_tris, rmd_grid_build **out) {
	if (!ctx) return rmd::fail(nullptr, RMD_ERR_INVALID_ARGUMENT, "rmd_grid_build_from_mesh_gpu: null context");
	if (!tri_pos || !tri_nrm || !out || n_tris == 0) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, "rmd_grid_build_from_mesh_gpu: null/empty input");
	if (n_tris >= (1ull << 32)) return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "rmd_grid_build_from_mesh_gpu: more than 2^32-1 triangles");
	std::unique_ptr<rmd_grid_build> g(new (std::nothrow) rmd_grid_build());
	if (!g) return rmd::fail(ctx, RMD_ERR_OUT_OF_MEMORY, "rmd_grid_build_from_mesh_gpu: allocation failed");
	rmd::mesh_bounds(tri_pos, n_tris, g->bbox_min, g->bbox_max); // on the host, in vertex order (header, step 1)
	// estimate_grid_resolution (acc_grid.rs:6-17) and cell_size (:38): same expressions, same libm as grid_build.cpp
	double size[3];
	for (int a = 0; a < 3; a++) size[a] = g->bbox_max[a] - g->bbox_min[a];
	const double volume = std::fabs(size[0] * size[1] * size[2]);
	const double density = std::pow((3.0 * (double)n_tris) / volume, 1.0 / 3.0);
	GridDims dims;
	for (int a = 0; a < 3; a++) {
		double v = std::fabs(size[a]) * density;
		uint64_t r = (!(v == v) || v <= 0.0) ? 0 : (v >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)v);
		if (r == 0 || r > 0xFFFFFFFFull)
			return rmd::fail(ctx, RMD_ERR_GRID_INDEX, "grid resolution has a zero axis (reference underflows `grid_res[i] - 1`, acc_grid.rs:54)");
		dims.res[a] = r, g->res[a] = (uint32_t)r;
		g->cell_size[a] = size[a] / (double)r;
		dims.bmin[a] = g->bbox_min[a], dims.cell[a] = g->cell_size[a];
	}
	dims.n_cells = dims.res[0] * dims.res[1] * dims.res[2];
	if (dims.n_cells > (1ull << 31)) return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "grid has more than 2^31 cells");

	RMD_HIP(ctx, hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	// (freed whichever way this function leaves; every size is at least one element — n_tris, n_cells >= 1 — but the mapping table's, which the device computes)
	rmd::DeviceBuffer pos_b, count_b, cells_b, sums_b, total_b, err_b, map_b;
	RMD_HIP(ctx, pos_b.alloc(n_tris * 9 * sizeof(double)));
	double *d_pos = pos_b.as<double>();
	RMD_HIP(ctx, hipMemcpyAsync(d_pos, tri_pos, n_tris * 9 * sizeof(double), hipMemcpyHostToDevice, st));
	const unsigned long long n_cells = dims.n_cells;
	const unsigned tri_blocks = (unsigned)((n_tris + 255) / 256), scan_blocks = (unsigned)((n_cells + 1023) / 1024);
	RMD_HIP(ctx, count_b.alloc(n_cells * sizeof(unsigned)));
	RMD_HIP(ctx, cells_b.alloc(n_cells * sizeof(unsigned)));
	RMD_HIP(ctx, sums_b.alloc(scan_blocks * sizeof(unsigned long long)));
	RMD_HIP(ctx, total_b.alloc(sizeof(unsigned long long)));
	RMD_HIP(ctx, err_b.alloc(sizeof(int)));
	unsigned *d_count = count_b.as<unsigned>(), *d_cells = cells_b.as<unsigned>();
	unsigned long long *d_sums = sums_b.as<unsigned long long>(), *d_total = total_b.as<unsigned long long>();
	int *d_err = err_b.as<int>();
	RMD_HIP(ctx, hipMemsetAsync(d_count, 0, n_cells * sizeof(unsigned), st));
	RMD_HIP(ctx, hipMemsetAsync(d_err, 0, sizeof(int), st));
	hipLaunchKernelGGL(scatter_kernel, dim3(tri_blocks), dim3(256), 0, st, 0, d_pos, (unsigned long long)n_tris, dims, d_count, (const unsigned *)nullptr,
	                   (unsigned *)nullptr, d_err);
	hipLaunchKernelGGL(scan_block_sums, dim3(scan_blocks), dim3(256), 0, st, d_count, n_cells, d_sums);
	hipLaunchKernelGGL(scan_of_sums, dim3(1), dim3(1), 0, st, d_sums, scan_blocks, d_total);
	RMD_HIP(ctx, hipGetLastError());
	unsigned long long total = 0;
	int err = 0;
	RMD_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, st));
	RMD_HIP(ctx, hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, st));
	RMD_HIP(ctx, hipStreamSynchronize(st));
	if (err == 1) return rmd::fail(ctx, RMD_ERR_GRID_INDEX, "cell bound does not fit usize (reference: \"Failed to cast cell bounds to usize\", acc_grid.rs:44-51)");
	if (err == 2) return rmd::fail(ctx, RMD_ERR_GRID_INDEX, "cell index past the cell array (reference panics at acc_grid.rs:61)");
	if (total > 0xFFFFFFFFull) return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, "mapping_table exceeds 2^32 entries");
	RMD_HIP(ctx, map_b.alloc(total ? total * sizeof(unsigned) : 16)); // (a 0-byte table allocates 16 bytes, as in rmd_scene_create)
	unsigned *d_map = map_b.as<unsigned>();
	hipLaunchKernelGGL(scan_write, dim3(scan_blocks), dim3(256), 0, st, d_count, n_cells, d_sums, d_cells, d_map);
	RMD_HIP(ctx, hipMemsetAsync(d_count, 0, n_cells * sizeof(unsigned), st)); // reused as the per-cell fill cursor
	hipLaunchKernelGGL(scatter_kernel, dim3(tri_blocks), dim3(256), 0, st, 1, d_pos, (unsigned long long)n_tris, dims, d_count, d_cells, d_map, d_err);
	hipLaunchKernelGGL(sort_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, st, d_cells, n_cells, d_map);
	RMD_HIP(ctx, hipGetLastError());
	g->cells.resize(n_cells);
	g->mapping.resize(total);
	RMD_HIP(ctx, hipMemcpyAsync(g->cells.data(), d_cells, n_cells * sizeof(unsigned), hipMemcpyDeviceToHost, st));
	RMD_HIP(ctx, hipMemcpyAsync(g->mapping.data(), d_map, total * sizeof(unsigned), hipMemcpyDeviceToHost, st));
	RMD_HIP(ctx, hipStreamSynchronize(st));
	g->pos.assign(tri_pos, tri_pos + n_tris * 9);
	g->nrm.assign(tri_nrm, tri_nrm + n_tris * 9);
	*out = g.release();
	return RMD_OK;
}
// (host vectors for the downloaded tables, device buffers behind RAII: nothing throws across the boundary)
extern "C" rmd_status rmd_grid_build_from_mesh_gpu(rmd_context *ctx, const double *tri_pos, const double *tri_nrm, uint64_t n_tris,
                                                   rmd_grid_build **out) {
	if (out) *out = nullptr;
	return rmd::guarded(ctx, "rmd_grid_build_from_mesh_gpu", [&] { return grid_build_from_mesh_gpu_impl(ctx, tri_pos, tri_nrm, n_tris, out); });
}
