// refine_core.h — the polisher hand-back (DESIGN.md §2 "Polisher hand-back"): what ccsx_refine.hip and ccsx_api.cpp share.  The error-probability table of the
// merged read quality, the parameter block of the three kernels, their launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CCSX_REFINE_NQ 94   // phred 0 .. 93

// perr_fx[q] = round(10^(-q / 10) x 2^32): literal constants, so that host, device and any other restatement add the same integers
#define CCSX_REFINE_PERR_TABLE                                                                                                     \
    4294967296ull, 3411613790ull, 2709941160ull, 2152582778ull, 1709857278ull, 1358187913ull, 1078847007ull, 856958639ull,         \
    680706443ull, 540704347ull, 429496730ull, 341161379ull, 270994116ull, 215258278ull, 170985728ull, 135818791ull,                \
    107884701ull, 85695864ull, 68070644ull, 54070435ull, 42949673ull, 34116138ull, 27099412ull, 21525828ull,                       \
    17098573ull, 13581879ull, 10788470ull, 8569586ull, 6807064ull, 5407043ull, 4294967ull, 3411614ull,                             \
    2709941ull, 2152583ull, 1709857ull, 1358188ull, 1078847ull, 856959ull, 680706ull, 540704ull,                                   \
    429497ull, 341161ull, 270994ull, 215258ull, 170986ull, 135819ull, 107885ull, 85696ull,                                         \
    68071ull, 54070ull, 42950ull, 34116ull, 27099ull, 21526ull, 17099ull, 13582ull,                                                \
    10788ull, 8570ull, 6807ull, 5407ull, 4295ull, 3412ull, 2710ull, 2153ull,                                                       \
    1710ull, 1358ull, 1079ull, 857ull, 681ull, 541ull, 429ull, 341ull,                                                             \
    271ull, 215ull, 171ull, 136ull, 108ull, 86ull, 68ull, 54ull,                                                                   \
    43ull, 34ull, 27ull, 22ull, 17ull, 14ull, 11ull, 9ull,                                                                         \
    7ull, 5ull, 4ull, 3ull, 3ull, 2ull

// the classes k_refine_check gives a tile, as bits (a tile may have several): the ZMW's code is -(lowest set bit's number + 1)
#define CCSX_REFINE_CLS_TILE   1u   // -1 BAD_TILE
#define CCSX_REFINE_CLS_ORDER  2u   // -2 BAD_ORDER
#define CCSX_REFINE_CLS_SYMBOL 4u   // -3 BAD_SYMBOL

#define CCSX_REFINE_THREADS 256     // k_refine_check: tiles per workgroup (one thread each)

// Everything the three kernels read and write.  The tile arrays, base_* and backbone are the slot's device copies of the caller's; draft / din_* are the slot's
// buffers k_draft_in reads afterwards; the rest is the report.
struct RefineParams {
    int32_t n_zmw, stride;             // U
    int64_t n_tiles;
    const int32_t *read_off;           // [n + 1] the batch's
    const int64_t *seq_off;            // [n + 1] the capacity layout
    const int32_t *tile_zmw, *tile_start, *tile_len, *tile_new_len;   // [n_tiles]
    const uint8_t *new_seq, *new_qual; // [n_tiles][U]
    const int32_t *base_len;           // [n] base.seq_len
    const uint8_t *base_seq, *base_qual;   // [capacity]
    const int32_t *backbone;           // [n]
    uint32_t *tile_cls;                // [n_tiles] CCSX_REFINE_CLS_* bits (k_refine_check)
    int32_t *counts;                   // [3] ZMWs with code 2, tiles applied, list-order violations; zeroed on the stream before the kernels
    int32_t *code, *n_applied, *new_len;   // [n] each
    int64_t *tile_first;               // [n] first tile of the ZMW's run (k_refine_plan, read by k_refine_splice)
    float *rq_merged;                  // [n]
    uint8_t *qual_merged;              // [capacity], or NULL: not asked for
    uint8_t *draft;                    // [capacity] = KParams::draft
    int32_t *din_len, *din_bb;         // [n] = KParams::din_len / din_bb
};

const char *ccsx_refine_launch(const RefineParams &R, hipStream_t st);   // ccsx_refine.hip: counts zeroed + the three kernels; NULL, or what failed
