// The edge arithmetic of the point-in-polygon kernels (k_points_in_polygon in amt_nearest.hip, k_scanline_select in
// amt_scanline.hip): matplotlib.path.Path(polygon).contains_points(points) (reference utils.py:58-74), the crossing test of a
// ray towards +x with the half-open edge rule (vertex y >= point y) of Agg's point_in_path.  ONE statement of it, so that both
// kernels give the same bits for the same point and edge: two products compared, nothing a contraction could fuse.
#ifndef AMT_POLYGON_H
#define AMT_POLYGON_H

#include <hip/hip_runtime.h>

namespace amt {

// the edge (x0, y0) -> (x1, y1) flips the point (tx, ty) between outside and inside
__device__ __forceinline__ bool polygon_edge_flips(double x0, double y0, double x1, double y1, double tx, double ty) {
    const bool f0 = y0 >= ty, f1 = y1 >= ty;
    return f0 != f1 && (((y1 - ty) * (x0 - x1) >= (x1 - tx) * (y0 - y1)) == f1);
}

// the edge can flip a point with ty in [lo, hi]: (y0 >= ty) != (y1 >= ty) needs a ty between the edge's ends
__device__ __forceinline__ bool polygon_edge_meets(double y0, double y1, double lo, double hi) {
    return fmax(y0, y1) >= lo && fmin(y0, y1) <= hi;
}

}  // namespace amt

#endif
