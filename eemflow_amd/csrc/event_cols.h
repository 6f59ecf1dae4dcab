// Reading the columns of an events npz in their file dtypes (the codes EEMFLOW_PACK_* of include/eemflow_hip.h): what event_pack.hip
// (columns -> the float64 table) and voxel_cols.hip (columns -> votes, no table) share.  Both files are built with -ffp-contract=off.
#pragma once

#include "common.h"

#include <cstdint>

namespace {

// element i of a column as astype(float64) gives it (the code is the same in every lane: a scalar branch).  Element-wise loads: a
// column may start at any element of its allocation
__device__ __forceinline__ double pk_load(const void* __restrict__ p, int code, long i) {
    switch (code) {
        case EEMFLOW_PACK_U8: return (double)static_cast<const uint8_t*>(p)[i];
        case EEMFLOW_PACK_I8: return (double)static_cast<const int8_t*>(p)[i];
        case EEMFLOW_PACK_U16: return (double)static_cast<const uint16_t*>(p)[i];
        case EEMFLOW_PACK_I16: return (double)static_cast<const int16_t*>(p)[i];
        case EEMFLOW_PACK_I32: return (double)static_cast<const int32_t*>(p)[i];
        case EEMFLOW_PACK_I64: return (double)static_cast<const long long*>(p)[i];       // round to nearest even
        case EEMFLOW_PACK_F32: return (double)static_cast<const float*>(p)[i];
        default: return static_cast<const double*>(p)[i];
    }
}

inline int pk_elem_bytes(int code) {
    switch (code) {
        case EEMFLOW_PACK_U8: case EEMFLOW_PACK_I8: return 1;
        case EEMFLOW_PACK_U16: case EEMFLOW_PACK_I16: return 2;
        case EEMFLOW_PACK_I32: case EEMFLOW_PACK_F32: return 4;
        case EEMFLOW_PACK_I64: case EEMFLOW_PACK_F64: return 8;
        default: return 0;
    }
}

}  // namespace
