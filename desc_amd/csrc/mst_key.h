// The edge order of the tree step (MPLS.m:160-193), shared by mst.hip and mst_batch.hip: the computed double fl(S_e + 1.0) first, then
// the edge's index in the (i, j)-sorted list.  That order is total, so the minimum spanning tree is unique.
#pragma once
#include "device_utils.h"

namespace desc {

// unsigned integer with the order of the double (positive: sign bit set; negative: all bits flipped)
__device__ __forceinline__ unsigned long long order_key(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}

}  // namespace desc
