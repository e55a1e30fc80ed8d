// Native vector types of the conv family (conv.hip, conv_identity.hip, conv1.hip, conv_os.hip, conv_dense.hip, conv_up.hip, conv_wide.hip, split.h,
// dense_tile.h): MFMA operands and accumulators, 16-byte loads and stores.  (Native vectors, not HIP's float4 / uint4
// structs: those copy as memcpy and stay in scratch.)
#pragma once

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
