// psm_grid_dev.h -- what the grid kernel files over a hierarchy share (grid.hip, grid_dist.hip): the kernel
// arguments of a grid, the voxel of a lane, the workgroups of a launch. Moved here from grid.hip as they were; grid.hip's kernels
// compile to the same instructions as with the pieces in their own file.
#pragma once
#include "psm_query_host.h"   // GridShape
#include "psm_query_dev.h"    // QUERY_BLOCK, QUERY_GRID_CAP

namespace psm {

namespace {

// (the walk's tree and its output are kernel parameters of their own, __restrict__: only then can the compiler tell that no
// store of the kernel changes a record or a triangle, and fetch them with scalar loads)
struct GridArgs {
    const uint32_t* sm;           // transform, leaf count, root
    const int32_t* sorted_tri;    // [0]: the lone leaf's triangle when the leaf count is 1
    float ox, oy, oz, cx, cy, cz; // psm_grid: origin, cell
    uint32_t nx, ny, nz;          // ... dims
    uint32_t nbx, nby;            // bricks along x and y
    uint32_t first, bricks;       // the bricks [first, first + bricks) are this launch's
    uint64_t* words;              // solid's fill: a word per brick of the whole grid
    float4* points;              // solid: the slab's centres, psm_point_query records in lane order
    const uint8_t* flags;         // solid: the slab's inside flags
};

// the voxel of lane `lane` in brick b, and whether it lies inside dims
struct Voxel {
    uint32_t ix, iy, iz;
    bool inside;
};
PSM_D Voxel voxel_of(const GridArgs& g, uint32_t b, int lane) {
    const uint32_t bx = b % g.nbx, t = b / g.nbx, by = t % g.nby, bz = t / g.nby;
    Voxel v;
    v.ix = 4u * bx + ((uint32_t)lane & 3u);
    v.iy = 4u * by + (((uint32_t)lane >> 2) & 3u);
    v.iz = 4u * bz + ((uint32_t)lane >> 4);
    v.inside = v.ix < g.nx && v.iy < g.ny && v.iz < g.nz;
    return v;
}

// the workgroups of a launch over `bricks` bricks: one per brick up to the cap, the rest by the kernels' grid-stride loops
inline uint32_t grid_for(uint64_t bricks) { return (uint32_t)(bricks < QUERY_GRID_CAP ? bricks : QUERY_GRID_CAP); }

// the grid's nine numbers and its bricks as the kernels take them
inline GridArgs grid_args(const psm_grid* grid, const GridShape& s) {
    GridArgs g = {};
    g.ox = grid->origin[0]; g.oy = grid->origin[1]; g.oz = grid->origin[2];
    g.cx = grid->cell[0]; g.cy = grid->cell[1]; g.cz = grid->cell[2];
    g.nx = grid->dims[0]; g.ny = grid->dims[1]; g.nz = grid->dims[2];
    g.nbx = s.nb[0]; g.nby = s.nb[1];
    g.first = 0u; g.bricks = (uint32_t)s.bricks;
    return g;
}

}  // namespace

}  // namespace psm
