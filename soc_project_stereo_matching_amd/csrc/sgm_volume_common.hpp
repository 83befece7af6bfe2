#pragma once
// What sgm_volume.hip and sgm_mesh.hip share: the volume as the kernels take it, a voxel's place and its centre, and, for the
// launchers, the one reading of a sgmd_volume.  Include after sgm_common.hpp.

struct VolumeParams {
    unsigned nx, ny, nz;
    unsigned n;                // voxels
    float voxel, ox, oy, oz, trunc;
    unsigned max_weight;
};

static __device__ __forceinline__ float volume_centre(float o, unsigned i, float voxel) { return o + ((float)i + 0.5f) * voxel; }

// n -> (i, j, k)
static __device__ __forceinline__ void volume_ijk(const VolumeParams& v, unsigned n, unsigned& i, unsigned& j, unsigned& k)
{
    const unsigned row = n / v.nx;
    i = n - row * v.nx;
    k = row / v.ny;
    j = row - k * v.ny;
}

// Corner c = dx | dy << 1 | dz << 2 of the cell whose corner 0 is voxel n; the edge of kind e (the mesh contract's table, whose
// kinds 0..2 are the axes of the surface list) runs from corner 0 to corner MESH_CORNER_OF(e)
#define MESH_CORNER_OF(e) ((e) == 0 ? 1 : (e) == 1 ? 2 : (e) == 2 ? 4 : (e) == 3 ? 3 : (e) == 4 ? 5 : (e) == 5 ? 6 : 7)

static bool volume_ok(const sgmd_volume* v)
{
    return v && v->nx >= 1 && v->ny >= 1 && v->nz >= 1 && v->nx <= 1024 && v->ny <= 1024 && v->nz <= 1024 &&
           (unsigned long long)v->nx * v->ny * v->nz <= (1ull << 30) && v->max_weight >= 1 && v->max_weight <= 65535;
}

static VolumeParams volume_params(const sgmd_volume* v)
{
    VolumeParams p;
    p.nx = (unsigned)v->nx; p.ny = (unsigned)v->ny; p.nz = (unsigned)v->nz;
    p.n = p.nx * p.ny * p.nz;
    p.voxel = v->voxel; p.ox = v->origin[0]; p.oy = v->origin[1]; p.oz = v->origin[2]; p.trunc = v->trunc;
    p.max_weight = v->max_weight;
    return p;
}
