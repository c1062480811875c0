// Fusion of depth maps into a truncated-signed-distance volume and the triangles of its zero level set.
//
// Every step of both is fp64 + - * / in a written order (the build has -ffp-contract=off), so a result is a matter of bytes:
// tests/tsdf_oracle.py states the same sequence in NumPy.  Every 3-term product sum is sfm_dense.h's dot3, and a voxel is projected
// into a view by that header's camera_matrices and project, as the depth filter projects a point.
//
// sfm_tsdf_integrate, 1 launch: one thread per voxel, x fastest, the loop over the views inside the thread.  The state (sum,
//   count, grey_sum) is read once and written once per call whatever the number of views; the view list, K and the poses are read
//   through wave-uniform addresses, a depth is one gather per voxel and view.  A voxel depends on no other voxel and adds its
//   views in the order of the list, so splitting the list over several calls gives the same bytes.
//
// sfm_tsdf_extract_mesh, 6 launches whatever the sizes, nothing read back: marching tetrahedra over the cells of the volume.
//   1. tsdf_count_kernel   one thread per cell: the triangles of its six tetrahedra (0 for a cell with a corner below min_count)
//   2-4. sfmorder::launch_scan   the exclusive scan of the counts (sfm_obs_order.h), the total behind the last cell
//   5. tsdf_emit_kernel    one thread per cell: its triangles to the rows the scan gave it, while they are below max_triangles
//   6. tsdf_tail_kernel    NaN into every row from the total on, and the total as int64
// A tetrahedron's corners are brought into the order "negative first, each group in the tetrahedron's own order" by six
// conditional swaps of registers, so nothing is indexed by a run-time value but global memory: no kernel uses scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_dense.h"
#include "sfm_obs_order.h"

namespace {

using sfmdense::dot3;
using sfmhost::aligned_to;
using sfmhost::check_launch;
using sfmhost::fail;
using sfmhost::grid_fits;
using sfmhost::grid_for;

constexpr int kBlock = 256;
constexpr int64_t kMaxTrianglesPerCell = 12;

struct Volume {
    int nx, ny, nz;
    double ox, oy, oz, s;
};

SFM_DEVICE double centre(double o, int i, double s) { return o + ((double)i + 0.5) * s; }

__global__ __launch_bounds__(kBlock) void tsdf_integrate_kernel(const Volume vol, double trunc, const double* __restrict__ depth,
                                                                const uint8_t* __restrict__ images, int64_t views, int H, int W,
                                                                const double* __restrict__ K, const double* __restrict__ poses,
                                                                const int32_t* __restrict__ list, int N, double* __restrict__ sum,
                                                                int32_t* __restrict__ count, int32_t* __restrict__ grey_sum,
                                                                int32_t* __restrict__ status) {
    if (blockIdx.x == 0)
        for (int n = threadIdx.x; n < N; n += kBlock) {
            const int32_t v = list[n];
            status[n] = v < 0 || (int64_t)v >= views ? SFM_TSDF_BAD_VIEW : SFM_TSDF_OK;
        }
    const int64_t voxels = (int64_t)vol.nx * vol.ny * vol.nz;
    const int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (l >= voxels) return;
    const int i = (int)(l % vol.nx), j = (int)((l / vol.nx) % vol.ny), k = (int)(l / ((int64_t)vol.nx * vol.ny));
    const double c[3] = {centre(vol.ox, i, vol.s), centre(vol.oy, j, vol.s), centre(vol.oz, k, vol.s)};
    sfmdense::Mat3 Km, Ki;   // only Km is used: the inverse folds away
    sfmdense::camera_matrices(K, Km, Ki);
    const int64_t plane = (int64_t)H * W;
    double acc = sum[l];
    int32_t seen = count[l];
    int32_t grey = grey_sum ? grey_sum[l] : 0;
    for (int n = 0; n < N; ++n) {
        const int32_t v = list[n];
        if (v < 0 || (int64_t)v >= views) continue;   // wave-uniform
        double u, w, z;
        sfmdense::project(Km, poses + (int64_t)v * 12, c, u, w, z);
        if (!(z > 0.0)) continue;
        const double x = floor(u + 0.5), y = floor(w + 0.5);
        if (!(x >= 0.0 && x < (double)W && y >= 0.0 && y < (double)H)) continue;
        const int64_t pixel = (int64_t)v * plane + (int64_t)(int)y * W + (int)x;
        const double d = depth[pixel];
        if (!(isfinite(d) && d > 0.0)) continue;
        const double sdf = d - z;
        if (sdf < -trunc) continue;
        const double f = sdf < trunc ? sdf / trunc : 1.0;
        acc = acc + f;
        seen = seen + 1;
        if (grey_sum) grey = grey + (int32_t)images[pixel];
    }
    sum[l] = acc;
    count[l] = seen;
    if (grey_sum) grey_sum[l] = grey;
}

// ---- marching tetrahedra ------------------------------------------------------------------------------------------------------
struct Corner {
    double f, g;
    int q;   // the corner of the cell, 0 .. 7: the linear voxel index grows with it
};

struct Cell {
    const double* sum;
    const int32_t *count, *grey_sum;
    int nx, ny;
    int i, j, k;
    int64_t base;   // the linear voxel index of corner 0
};

SFM_DEVICE int64_t corner_voxel(const Cell& c, int q) {
    return c.base + (q & 1) + (int64_t)((q >> 1) & 1) * c.nx + (int64_t)((q >> 2) & 1) * c.nx * c.ny;
}

SFM_DEVICE bool cell_valid(const Cell& c, int min_count) {
    bool valid = true;
#pragma unroll
    for (int q = 0; q < 8; ++q) valid = valid && c.count[corner_voxel(c, q)] >= min_count;
    return valid;
}

SFM_DEVICE Corner load_corner(const Cell& c, int q) {
    const int64_t l = corner_voxel(c, q);
    const double n = (double)c.count[l];
    Corner r;
    r.f = c.sum[l] / n;
    r.g = c.grey_sum ? (double)c.grey_sum[l] / n : 0.0;
    r.q = q;
    return r;
}

// negative corners in front of the others, both groups in the order they came in; -> the number of negative corners
SFM_DEVICE int negatives_first(Corner& e0, Corner& e1, Corner& e2, Corner& e3) {
#define SFM_TSDF_SWAP(a, b)                      \
    if (!(a.f < 0.0) && b.f < 0.0) {             \
        const Corner t = a;                      \
        a = b;                                   \
        b = t;                                   \
    }
    SFM_TSDF_SWAP(e0, e1) SFM_TSDF_SWAP(e1, e2) SFM_TSDF_SWAP(e2, e3)
    SFM_TSDF_SWAP(e0, e1) SFM_TSDF_SWAP(e1, e2)
    SFM_TSDF_SWAP(e0, e1)
#undef SFM_TSDF_SWAP
    return (e0.f < 0.0) + (e1.f < 0.0) + (e2.f < 0.0) + (e3.f < 0.0);
}

SFM_DEVICE int triangles_of(int negatives) { return negatives == 2 ? 2 : (negatives == 1 || negatives == 3 ? 1 : 0); }

struct Vertex {
    double x, y, z, g;
};

SFM_DEVICE Vertex edge_vertex(const Volume& vol, const Cell& c, const Corner& p, const Corner& q) {
    const bool p_low = p.q < q.q;
    const double lf = p_low ? p.f : q.f, hf = p_low ? q.f : p.f, lg = p_low ? p.g : q.g, hg = p_low ? q.g : p.g;
    const int lq = p_low ? p.q : q.q, hq = p_low ? q.q : p.q;
    const double t = lf / (lf - hf);
    const double lx = centre(vol.ox, c.i + (lq & 1), vol.s), hx = centre(vol.ox, c.i + (hq & 1), vol.s);
    const double ly = centre(vol.oy, c.j + ((lq >> 1) & 1), vol.s), hy = centre(vol.oy, c.j + ((hq >> 1) & 1), vol.s);
    const double lz = centre(vol.oz, c.k + ((lq >> 2) & 1), vol.s), hz = centre(vol.oz, c.k + ((hq >> 2) & 1), vol.s);
    Vertex v;
    v.x = lx + t * (hx - lx);
    v.y = ly + t * (hy - ly);
    v.z = lz + t * (hz - lz);
    v.g = lg + t * (hg - lg);
    return v;
}

struct MeshOut {
    double *vertices, *grey;
    int64_t max_triangles;
};

SFM_DEVICE void store_triangle(const MeshOut& out, int64_t row, const Vertex& A, Vertex B, Vertex C, double D0, double D1, double D2) {
    if (row >= out.max_triangles) return;
    const double a0 = B.x - A.x, a1 = B.y - A.y, a2 = B.z - A.z;
    const double b0 = C.x - A.x, b1 = C.y - A.y, b2 = C.z - A.z;
    const double n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
    if (dot3(n0, D0, n1, D1, n2, D2) < 0.0) {
        const Vertex t = B;
        B = C;
        C = t;
    }
    double* v = out.vertices + row * 9;
    v[0] = A.x, v[1] = A.y, v[2] = A.z;
    v[3] = B.x, v[4] = B.y, v[5] = B.z;
    v[6] = C.x, v[7] = C.y, v[8] = C.z;
    if (out.grey) {
        double* g = out.grey + row * 3;
        g[0] = A.g, g[1] = B.g, g[2] = C.g;
    }
}

// the sum of one coordinate bit over the corners of a group
SFM_DEVICE int bit_sum(int shift, int qa, int qb, int qc) { return ((qa >> shift) & 1) + ((qb >> shift) & 1) + ((qc >> shift) & 1); }

// The triangles of one tetrahedron (its corners in the tetrahedron's order) to the rows from `row` on; -> their number.
// kEmit = false only counts.
template <bool kEmit>
SFM_DEVICE int tetrahedron(const Volume& vol, const Cell& c, Corner e0, Corner e1, Corner e2, Corner e3, const MeshOut& out, int64_t row) {
    const int negatives = negatives_first(e0, e1, e2, e3);
    const int triangles = triangles_of(negatives);
    if (!kEmit || triangles == 0) return triangles;
    // D = n_neg (sum of the non-negative corners' indices) - n_pos (sum of the negative corners'): the cell's own index cancels
    double D[3];
    if (negatives == 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) D[a] = (double)(bit_sum(a, e1.q, e2.q, e3.q) - 3 * ((e0.q >> a) & 1));
        store_triangle(out, row, edge_vertex(vol, c, e0, e1), edge_vertex(vol, c, e0, e2), edge_vertex(vol, c, e0, e3), D[0], D[1], D[2]);
    } else if (negatives == 3) {
#pragma unroll
        for (int a = 0; a < 3; ++a) D[a] = (double)(3 * ((e3.q >> a) & 1) - bit_sum(a, e0.q, e1.q, e2.q));
        store_triangle(out, row, edge_vertex(vol, c, e3, e0), edge_vertex(vol, c, e3, e1), edge_vertex(vol, c, e3, e2), D[0], D[1], D[2]);
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a)
            D[a] = (double)(2 * (((e2.q >> a) & 1) + ((e3.q >> a) & 1)) - 2 * (((e0.q >> a) & 1) + ((e1.q >> a) & 1)));
        const Vertex ac = edge_vertex(vol, c, e0, e2), bd = edge_vertex(vol, c, e1, e3);
        store_triangle(out, row, ac, edge_vertex(vol, c, e0, e3), bd, D[0], D[1], D[2]);
        store_triangle(out, row + 1, ac, bd, edge_vertex(vol, c, e1, e2), D[0], D[1], D[2]);
    }
    return triangles;
}

// the six tetrahedra of the Kuhn split about the diagonal 0-7, in the order of the definition; -> the triangles of the cell
template <bool kEmit>
SFM_DEVICE int march_cell(const Volume& vol, const Cell& c, const MeshOut& out, int64_t row) {
    const Corner c0 = load_corner(c, 0), c1 = load_corner(c, 1), c2 = load_corner(c, 2), c3 = load_corner(c, 3);
    const Corner c4 = load_corner(c, 4), c5 = load_corner(c, 5), c6 = load_corner(c, 6), c7 = load_corner(c, 7);
    int n = 0;
    n += tetrahedron<kEmit>(vol, c, c0, c1, c3, c7, out, row + n);
    n += tetrahedron<kEmit>(vol, c, c0, c3, c2, c7, out, row + n);
    n += tetrahedron<kEmit>(vol, c, c0, c2, c6, c7, out, row + n);
    n += tetrahedron<kEmit>(vol, c, c0, c6, c4, c7, out, row + n);
    n += tetrahedron<kEmit>(vol, c, c0, c4, c5, c7, out, row + n);
    n += tetrahedron<kEmit>(vol, c, c0, c5, c1, c7, out, row + n);
    return n;
}

SFM_DEVICE Cell cell_of(const Volume& vol, int64_t cell, const double* sum, const int32_t* count, const int32_t* grey_sum) {
    const int cxn = vol.nx - 1, cyn = vol.ny - 1;
    Cell c;
    c.sum = sum, c.count = count, c.grey_sum = grey_sum, c.nx = vol.nx, c.ny = vol.ny;
    c.i = (int)(cell % cxn), c.j = (int)((cell / cxn) % cyn), c.k = (int)(cell / ((int64_t)cxn * cyn));
    c.base = ((int64_t)c.k * vol.ny + c.j) * vol.nx + c.i;
    return c;
}

__global__ __launch_bounds__(kBlock) void tsdf_count_kernel(const Volume vol, int64_t cells, const double* __restrict__ sum,
                                                            const int32_t* __restrict__ count, int min_count,
                                                            int32_t* __restrict__ counts, int32_t* __restrict__ flag) {
    const int64_t cell = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell == 0) *flag = 0;   // the scan's launches return at once on a set flag: the workspace comes as it is
    if (cell >= cells) return;
    const Cell c = cell_of(vol, cell, sum, count, nullptr);
    const MeshOut none{nullptr, nullptr, 0};
    counts[cell] = cell_valid(c, min_count) ? march_cell<false>(vol, c, none, 0) : 0;
}

__global__ __launch_bounds__(kBlock) void tsdf_emit_kernel(const Volume vol, int64_t cells, const double* __restrict__ sum,
                                                           const int32_t* __restrict__ count, const int32_t* __restrict__ grey_sum,
                                                           const int32_t* __restrict__ offsets, const MeshOut out) {
    const int64_t cell = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= cells) return;
    const int64_t row = offsets[cell];
    if (offsets[cell + 1] == row || row >= out.max_triangles) return;
    const Cell c = cell_of(vol, cell, sum, count, grey_sum);
    march_cell<true>(vol, c, out, row);
}

__global__ __launch_bounds__(kBlock) void tsdf_tail_kernel(const int32_t* __restrict__ offsets, int64_t cells, const MeshOut out,
                                                           int64_t* __restrict__ total) {
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t found = offsets[cells];
    if (row == 0) *total = found;
    if (row < found || row >= out.max_triangles) return;
#pragma unroll
    for (int a = 0; a < 9; ++a) out.vertices[row * 9 + a] = NAN;
    if (out.grey)
#pragma unroll
        for (int a = 0; a < 3; ++a) out.grey[row * 3 + a] = NAN;
}

bool volume_sizes_ok(int64_t nx, int64_t ny, int64_t nz, int64_t least) {
    const int64_t limit = (int64_t)1 << 31;
    return nx >= least && ny >= least && nz >= least && nx < limit && ny < limit && nz < limit && nx * ny < limit && nx * ny * nz < limit;
}

bool volume_scalars_ok(double ox, double oy, double oz, double s) { return isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(s) && s > 0.0; }

// int32 offsets hold every cell's triangles
bool mesh_sizes_ok(int64_t nx, int64_t ny, int64_t nz) {
    return volume_sizes_ok(nx, ny, nz, 2) && (nx - 1) * (ny - 1) * (nz - 1) * kMaxTrianglesPerCell < ((int64_t)1 << 31);
}

struct MeshWorkspace {
    int32_t *counts, *tile_sum, *flag;
    int64_t bytes;
};

MeshWorkspace carve_mesh(void* base, int64_t cells) {
    sfmhost::Carver c{(uintptr_t)base, 0};
    MeshWorkspace w;
    w.counts = c.take<int32_t>(cells + 1);
    w.tile_sum = c.take<int32_t>(sfmorder::tiles(cells));
    w.flag = c.take<int32_t>(1);
    w.bytes = c.at;
    return w;
}

}  // namespace

extern "C" {

int sfm_tsdf_integrate(double* sum, int32_t* count, int32_t* grey_sum, int64_t nx, int64_t ny, int64_t nz, double ox, double oy, double oz,
                       double voxel_size, double truncation, const double* depth, const uint8_t* images, int64_t views, int64_t height,
                       int64_t width, const double* K, const double* poses, const int32_t* view_list, int64_t view_count, int32_t* status,
                       void* stream) {
    // every check before the launch: a refused call has enqueued nothing
    if (!volume_sizes_ok(nx, ny, nz, 1)) return fail(SFM_EINVAL, "sfm_tsdf_integrate: need nx, ny, nz >= 1 and nx * ny * nz < 2^31");
    if (!volume_scalars_ok(ox, oy, oz, voxel_size) || !isfinite(truncation) || !(truncation > 0.0))
        return fail(SFM_EINVAL, "sfm_tsdf_integrate: the origin must be finite, voxel_size and truncation finite and > 0");
    if (!sfmhost::image_stack_ok(views, height, width))
        return fail(SFM_EINVAL, "sfm_tsdf_integrate: need 1 <= views < 2^31 and 1 <= height * width < 2^31");
    if (view_count < 0 || view_count > 0x7FFFFFFF) return fail(SFM_EINVAL, "sfm_tsdf_integrate: need 0 <= view_count < 2^31");
    if (!grid_fits(nx * ny * nz, kBlock, kBlock))
        return fail(SFM_EINVAL, "sfm_tsdf_integrate: size exceeds what one launch covers (2^31-1 blocks, 2^32-1 threads in x)");
    if ((images == nullptr) != (grey_sum == nullptr))
        return fail(SFM_EINVAL, "sfm_tsdf_integrate: images must be NULL exactly when grey_sum is NULL");
    if (!sum || !count || !depth || !K || !poses) return fail(SFM_EINVAL, "sfm_tsdf_integrate: null pointer");
    if (!aligned_to(sum, 8) || !aligned_to(depth, 8) || !aligned_to(K, 8) || !aligned_to(poses, 8) || !aligned_to(count, 4) ||
        !aligned_to(grey_sum, 4) || !aligned_to(view_list, 4) || !aligned_to(status, 4))
        return fail(SFM_EINVAL, "sfm_tsdf_integrate: misaligned pointer (doubles 8, int32 4 bytes)");
    if (view_count == 0) return SFM_OK;
    if (!view_list || !status) return fail(SFM_EINVAL, "sfm_tsdf_integrate: null pointer");
    const Volume vol{(int)nx, (int)ny, (int)nz, ox, oy, oz, voxel_size};
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(grid_for(nx * ny * nz, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, vol, truncation,
                       depth, images, views, (int)height, (int)width, K, poses, view_list, (int)view_count, sum, count, grey_sum, status);
    return check_launch("sfm_tsdf_integrate");
}

int64_t sfm_tsdf_mesh_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    return mesh_sizes_ok(nx, ny, nz) ? carve_mesh(nullptr, (nx - 1) * (ny - 1) * (nz - 1)).bytes : -1;
}

int sfm_tsdf_extract_mesh(const double* sum, const int32_t* count, const int32_t* grey_sum, int64_t nx, int64_t ny, int64_t nz, double ox,
                          double oy, double oz, double voxel_size, int min_count, int64_t max_triangles, double* vertices, double* grey,
                          int64_t* total, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!mesh_sizes_ok(nx, ny, nz))
        return fail(SFM_EINVAL, "sfm_tsdf_extract_mesh: need nx, ny, nz >= 2, nx * ny * nz < 2^31 and 12 (nx-1)(ny-1)(nz-1) < 2^31");
    if (!volume_scalars_ok(ox, oy, oz, voxel_size)) return fail(SFM_EINVAL, "sfm_tsdf_extract_mesh: the origin must be finite, voxel_size finite and > 0");
    if (min_count < 1) return fail(SFM_EINVAL, "sfm_tsdf_extract_mesh: need min_count >= 1");
    if (max_triangles < 0 || max_triangles > ((int64_t)1 << 40)) return fail(SFM_EINVAL, "sfm_tsdf_extract_mesh: need 0 <= max_triangles <= 2^40");
    const int64_t cells = (nx - 1) * (ny - 1) * (nz - 1);
    if (!grid_fits(cells, kBlock, kBlock) || !grid_fits(max_triangles, kBlock, kBlock))
        return fail(SFM_EINVAL, "sfm_tsdf_extract_mesh: size exceeds what one launch covers (2^31-1 blocks, 2^32-1 threads in x)");
    if ((grey == nullptr) != (grey_sum == nullptr) && max_triangles > 0)
        return fail(SFM_EINVAL, "sfm_tsdf_extract_mesh: grey must be NULL exactly when grey_sum is NULL");
    if (!sum || !count || !total || !workspace || (max_triangles > 0 && !vertices)) return fail(SFM_EINVAL, "sfm_tsdf_extract_mesh: null pointer");
    if (!aligned_to(sum, 8) || !aligned_to(vertices, 8) || !aligned_to(grey, 8) || !aligned_to(total, 8) || !aligned_to(count, 4) ||
        !aligned_to(grey_sum, 4) || !aligned_to(workspace, 16))
        return fail(SFM_EINVAL, "sfm_tsdf_extract_mesh: misaligned pointer (doubles and total 8, int32 4, the workspace 16 bytes)");
    const MeshWorkspace w = carve_mesh(workspace, cells);
    if (workspace_bytes < w.bytes) return fail(SFM_EINVAL, "sfm_tsdf_extract_mesh: workspace too small (sfm_tsdf_mesh_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const Volume vol{(int)nx, (int)ny, (int)nz, ox, oy, oz, voxel_size};
    const MeshOut out{vertices, max_triangles > 0 ? grey : nullptr, max_triangles};
    const dim3 cell_grid(grid_for(cells, kBlock));
    hipLaunchKernelGGL(tsdf_count_kernel, cell_grid, dim3(kBlock), 0, st, vol, cells, sum, count, min_count, w.counts, w.flag);
    sfmorder::launch_scan(w.counts, cells, w.tile_sum, w.flag, st);
    hipLaunchKernelGGL(tsdf_emit_kernel, cell_grid, dim3(kBlock), 0, st, vol, cells, sum, count, grey_sum, w.counts, out);
    hipLaunchKernelGGL(tsdf_tail_kernel, dim3(grid_for(max_triangles, kBlock)), dim3(kBlock), 0, st, w.counts, cells, out, total);
    return check_launch("sfm_tsdf_extract_mesh");
}

}  // extern "C"
