// hdb_mfma_ksplit.hip -- the MFMA row scan for rows too wide for one wave's query fragments: float32 d = 1024 / 1536 (the
// reference's default precision at its demo width, hyperdb.py:51), fp16 d = 2048 / 3072 / 4096, bfloat16 d = 640 .. 4096 and, on
// request (f8_ks_min_q, b1_mfma_min_q), float8 e4m3 and packed-bit rows d = 640 .. 4096.
//
// A wave holds the B fragments of 16 queries for at most 3072 bytes of row (192 registers; bfloat16 rows, whose float32 queries
// travel as three bf16 parts: 1024 bytes), and a 16-row LDS stage of wider rows does not fit the 3-deep ring.  So the K dimension
// is cut into S slices that the EXISTING slice geometries cover (ks_geom, hdb_caps.h: float32 512 / 768 elements, fp16 1024 /
// 1536, bfloat16 512 / 384 / 256 -- the slices of one row may differ in width): one launch per slice reads its piece of every row
// (row pitch = the full row), starts its accumulators from the sums of the slices before (a [query][rows] float32 buffer, the
// layout of MODE 0's scores) and either stores the raw sums for the next slice (MODE 3) or, in the last slice, runs the metric's
// epilogue as usual (scores or threshold filter).  V is still read exactly once per pass; the partial sums add 8 B per row, query
// and extra slice (Q = 64, float32 d = 1536: +8 % traffic).  Batches of 5-128 queries per pass instead of the VALU scan's 4 (a
// 256-query batch on a float32 d = 1536 matrix: 2 x 2 launches instead of 64 passes).
#include "hdb_mfma_kernel.h"

// args->ks_partial_out: [nq_launch][ks_ld] float32 scratch of the caller (MODE 0 passes may alias it with args->scores: the last
// slice overwrites the sums with the scores, element by element, by the lane that read them)
// l: the launch as the router built it (mode: the last slice's; qscl: nullptr for every row type but fp16, whose queries alone are
// scaled copies); every slice gets a copy with its own mode and width
extern "C" int hdb_launch_mfma_ksplit(const ScanArgs* args, int dtype, const MfmaLaunch* l) {
    const KsGeom g = dtype == HDB_F8E4M3 ? ks_geom_f8(args->d) : dtype == HDB_B1 ? ks_geom_b1(args->d) : ks_geom(dtype, args->d);       // (float8, packed bits: the opt-in lists, no part of ks_geom)
    if (!g.slices || !args->ks_partial_out) return (int)hipErrorInvalidValue;
    for (int s = 0; s < g.slices; ++s) {
        ScanArgs a = *args;
        a.ks_pitch = hdb_row_bytes(dtype, args->d); a.ks_off = g.off[s]; a.ks_dfull = args->d;
        if (dtype == HDB_B1) a.ks_off = g.off[s] * 8;         // (packed bits: the kernel takes the ELEMENT offset -- into the query as it is, an eighth of it into the row)
        a.ks_partial_in = s == 0 ? nullptr : args->ks_partial_out;
        MfmaLaunch sl = *l;
        sl.mode = s + 1 < g.slices ? 3 : l->mode;
        sl.width = g.width[s];
        int rc;
        if (dtype == HDB_F8E4M3 && args->f8_lds) rc = hdb_launch_mfma_kslice_f8_lds(&a, &sl);       // (blocks: a limit, each slice sizes its own grid)
        else if (dtype == HDB_F8E4M3) rc = hdb_launch_mfma_kslice_f8(&a, &sl);
        else if (dtype == HDB_B1) rc = hdb_launch_mfma_kslice_b1(&a, &sl);
        else if (dtype == HDB_BF16) rc = hdb_launch_mfma_kslice_bf16(&a, &sl);
        else if (dtype == HDB_F32 && args->f32_split) rc = hdb_launch_mfma_kslice_f32s(&a, &sl);
        else if (dtype == HDB_F32) rc = sl.width == 512 ? launch_kslice<float, 512, 16>(a, sl) : launch_kslice<float, 768, 16>(a, sl);
        else rc = sl.width == 1024 ? launch_kslice<_Float16, 1024, 16>(a, sl) : launch_kslice<_Float16, 1536, 16>(a, sl);
        if (rc) return rc;
    }
    return 0;
}
