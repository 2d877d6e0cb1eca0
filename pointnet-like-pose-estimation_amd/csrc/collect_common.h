// collect_common.h -- what the camera-cloud units (collect.hip, knn.hip, plane.hip) share: the size limit,
// the distance of include/pn2.h rule 2, the row loader and the argument checks of every entry.
#pragma once
#include "pn2_internal.h"

namespace pn2 {

constexpr int64_t kCollectMaxN = (int64_t)1 << 20;

// ------------------------------------------------------------------------ the neighbour rule
// d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float64, every operation rounded once.
__device__ __forceinline__ double nbr_d2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

template <typename T>
__device__ __forceinline__ void load_xyz(const T *pts, int64_t ld, int64_t row, double &x, double &y, double &z) {
    const T *p = pts + row * ld;
    x = (double)p[0], y = (double)p[1], z = (double)p[2];
}

static int64_t elem_size(int dtype) { return dtype == PN2_DTYPE_F64 ? 8 : dtype == PN2_DTYPE_F32 ? 4 : 0; }
static int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

// the checks every entry shares: 0 to go on, else the code to return
static int check_cloud(const char *who, const void *pts, int dtype, int64_t N, int64_t C, int64_t ld) {
    PN2_REQUIRE(pts, "%s: null pointer", who);
    PN2_REQUIRE(elem_size(dtype) != 0, "%s: unknown dtype %d", who, dtype);
    PN2_REQUIRE(N >= 0 && C >= 3 && C <= kMaxCWide && ld >= C, "%s: bad shape (N=%lld C=%lld ld=%lld; 3 <= C <= 64)",
                who, (long long)N, (long long)C, (long long)ld);
    if (N > kCollectMaxN)
        return set_error(PN2_EUNSUPPORTED, "%s: N=%lld above pn2_collect_max_points() = %lld", who, (long long)N,
                         (long long)kCollectMaxN);
    return PN2_OK;
}

}  // namespace pn2
