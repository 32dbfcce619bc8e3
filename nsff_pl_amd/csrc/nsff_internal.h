// Entry points of the fp16-split field path (field_h3.hip), dispatched from the C-ABI in field.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/nsff_render.h"

int nsff_h3_packed_bytes(const NsffModelDesc* desc, size_t* bytes);
int nsff_h3_pack_weights(const NsffModelDesc* desc, const float* const* params, void* packed, bool fold, hipStream_t st);
int nsff_h3_fold_heads(const NsffModelDesc* desc, const float* const* params, void* packed, hipStream_t st);
int nsff_fold_rows_f32(const NsffModelDesc* desc, const float* const* params, float* s_w, float* s_b, float* t_w, float* t_b,
                       hipStream_t st);
// args already validated by nsff_field_query; points_per_block is 64 / 130 / 131 (the f16x3 tilings of NsffFieldArgs::tile_points)
// span (or null, profiling): NSFF_SPAN_WORDS zeroed uint64 that receive the summed lifetimes of a sample of the launch's
// workgroups in shader-clock ticks [0] and in wall-clock ticks [1]
#define NSFF_SPAN_WORDS 2
int nsff_h3_field_query(const NsffModelDesc* desc, const void* packed, const NsffFieldArgs* args,
                        int points_per_block, hipStream_t st, unsigned long long* span = nullptr, const void* repacked = nullptr);
// the 16x16x32 form of the hand-scheduled inference kernel (nsff_field_kernel_h3a16): its packed buffer from the f16x3 pack, the shape
// a launch would run (host-only), the shape the last f16x3 launch ran
int nsff_h3_repack_weights(const NsffModelDesc* desc, const void* packed, void* repacked, hipStream_t st);
int nsff_h3_field_mfma_shape(const NsffModelDesc* desc, const NsffFieldArgs* args);
extern int g_nsff_last_h3_shape;

// the library's choice of points_per_block (NsffFieldArgs::tile_points = 0): 128 points as eight waves of 32 neurons (one
// workgroup per CU, every weight byte fetched once per 128 points, no spilled registers: 41 MB instead of 79 MB of HBM traffic
// per C2 launch and -0.8 % time); launches too small to give every CU such a tile keep the 64-point tiling (two workgroups per CU)
inline int nsff_h3_default_tile(long long n_points) { return n_points >= 128LL * 256 ? 130 : 64; }

extern int g_nsff_last_h3_kernel;
extern int g_nsff_last_h3_grid;
