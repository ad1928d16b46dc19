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
extern "C" int hdb_launch_mfma_ksplit(const ScanArgs* args, int dtype, int mode, int nq_launch, const void* q, const float* sqnorm,
                                      const float* qsq, const float* qscl, int blocks, void* stream) {
    const KsGeom g = dtype == HDB_F8E4M3 ? ks_geom_f8(args->d) : dtype == HDB_B1 ? ks_geom_b1(args->d) : ks_geom(dtype, args->d);       // (float8, packed bits: the opt-in lists, no part of ks_geom)
    if (!g.slices || !args->ks_partial_out) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    for (int s = 0; s < g.slices; ++s) {
        ScanArgs a = *args;
        a.ks_pitch = hdb_row_bytes(dtype, args->d); a.ks_off = g.off[s]; a.ks_dfull = args->d;
        if (dtype == HDB_B1) a.ks_off = g.off[s] * 8;         // (packed bits: the kernel takes the ELEMENT offset -- into the query as it is, an eighth of it into the row)
        a.ks_partial_in = s == 0 ? nullptr : args->ks_partial_out;
        const int m = s + 1 < g.slices ? 3 : mode;
        const int w = g.width[s];
        int rc;
        if (dtype == HDB_F8E4M3 && args->f8_lds) rc = hdb_launch_mfma_kslice_f8_lds(&a, w, m, nq_launch, q, sqnorm, qsq, blocks, stream);       // (blocks: a limit, each slice sizes its own grid)
        else if (dtype == HDB_F8E4M3) rc = hdb_launch_mfma_kslice_f8(&a, w, m, nq_launch, q, sqnorm, qsq, blocks, stream);
        else if (dtype == HDB_B1) rc = hdb_launch_mfma_kslice_b1(&a, w, m, nq_launch, q, sqnorm, qsq, blocks, stream);
        else if (dtype == HDB_BF16) rc = hdb_launch_mfma_kslice_bf16(&a, w, m, nq_launch, q, sqnorm, qsq, blocks, stream);       // (float32 queries as they are: no qscl)
        else if (dtype == HDB_F32 && args->f32_split) rc = hdb_launch_mfma_kslice_f32s(&a, w, m, nq_launch, q, sqnorm, qsq, blocks, stream);
        else if (dtype == HDB_F32) rc = w == 512 ? launch_kslice<float, 512, 16>(a, m, q, sqnorm, qsq, nullptr, nq_launch, blocks, st)
                                                 : launch_kslice<float, 768, 16>(a, m, q, sqnorm, qsq, nullptr, nq_launch, blocks, st);
        else rc = w == 1024 ? launch_kslice<_Float16, 1024, 16>(a, m, q, sqnorm, qsq, qscl, nq_launch, blocks, st)
                            : launch_kslice<_Float16, 1536, 16>(a, m, q, sqnorm, qsq, qscl, nq_launch, blocks, st);
        if (rc) return rc;
    }
    return 0;
}
