// dw_plan.h -- the GPU-free part of the weight-gradient launch (backward.hip): the argument blocks of the two launches, the
// table of job shapes, and the plan that turns the products of one model into jobs, workgroup shares and slab places.
// Nothing here calls HIP; tools/dw_plan_check.cpp runs it stand-alone.
//
// Every weight-gradient product of one model's backward pass leaves in ONE launch (dw_multi_kernel, or dw_multi_split_kernel
// in split precision), and their reductions in a second one (dw_reduce_multi_kernel): a job owns a range of workgroups sized
// to what its shape costs per chunk, DW_GRID workgroups in all -- one per CU from the first chunk to the last, all products in
// flight together (no ramp and tail per product, ~23 slabs per product to reduce, and 2 launches per model on a step that is
// host-bound at the reference's batch size).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/nerf_amd.h"

namespace na {

enum { PERM_NAT = 0, PERM_ACC = 1, PERM_GEN = 2 };     // slot order of a row: natural, the accumulator's, the generated encoding's

struct DwArgs {
    const uint16_t *G; int ldg;          // [P, ldg] bf16 gradient rows, columns [0, 16*OT) used
    const uint16_t *X; int ldx;          // [P, ldx] bf16 activation rows, columns [0, 16*IT) used
    int64_t P;
    float *slab;                         // per-workgroup partial results: [grid][OT*IT*256 + OT*16 (+ IT*256 + 16 with a head)] fp32
    const uint16_t *H;                   // head gradients transposed inside 32-point chunks (kernels.h g_rawt), or NULL
    // split-precision products (dw2s_body): the planes of fp16 lo rows of G, X and H (the pointers above are the hi planes)
    const uint16_t *G_lo, *X_lo, *H_lo;
};

struct DwReduceArgs {
    const float *slab; int n_slabs, OT, IT;
    float *dW; int ld_dw, col_off;       // nn.Linear weight gradient [n_out][ld_dw], written at column col_off + feature
    float *db;                           // bias gradient [n_out] or NULL
    int out_kind, in_kind, in_L, n_valid, m_valid;
    // a head product riding on this job (same X): one more 16-row tile whose rows are the columns of dL/draw; rows
    // [head_row0, head_row0 + head_rows) of it are the head's weight gradient [head_rows][head_ld] (+ bias gradient)
    int HT;                              // 0 or 1
    float *head_dW, *head_db;
    int head_row0, head_rows, head_ld;
    const float *inv_scale;              // split precision: 1 / loss scale (a device scalar, split.h), or NULL
};
constexpr int dw_slab_floats(int OT, int IT, int HT) { return OT * IT * 256 + OT * 16 + HT * (IT * 256 + 16); }

constexpr int DW_GRID = 256;             // workgroups of the one launch
constexpr int DW_MAX_JOBS = 16;
constexpr int DWR_BLOCK = 512;           // elements of a job's summed slabs per reduction block
struct DwJob {
    DwArgs a;
    int shape;                           // row of DW_SHAPE
    int first_block, n_blocks;
};
struct DwMulti {
    DwJob job[DW_MAX_JOBS];
    int n;
};
struct DwReduceMulti {
    DwReduceArgs r[DW_MAX_JOBS];
    int first_block[DW_MAX_JOBS + 1];
    int n;
};

// Ring slots of a streaming body: what fits in 128 KiB, at least 4 (split: 2, its chunk image is twice as large) and at
// most 12 -- a narrow product keeps as many BYTES in flight as a wide one.
constexpr int DW2_NS(int OT, int IT) {
    const int n = (128 * 1024) / (32 * 32 * (OT + IT));
    return n < 4 ? 4 : (n > 12 ? 12 : n);
}
constexpr int DW2S_NS(int OT, int IT) {
    const int n = (128 * 1024) / (2 * 32 * 32 * (OT + IT));
    return n < 2 ? 2 : (n > 12 ? 12 : n);
}
constexpr size_t dw_split_lds(int OT, int IT, bool head) { return (size_t)DW2S_NS(OT, IT) * (2 * 32 * 32 * (OT + IT) + (head ? 2048 : 0)); }
constexpr size_t dw_bf16_lds(int OT, int IT, bool head) { return (size_t)DW2_NS(OT, IT) * (32 * 32 * (OT + IT) + (head ? 1024 : 0)); }

// The job shapes, stated once: the body a job runs is dw2_body / dw2s_body<OT, IT, WO, WI, HEAD> (OT / IT: 16-wide tiles of
// the output / input feature axis, the 8 waves as a WO x WI grid, HEAD: a head product rides along), or for OT == 0 the head
// alone on IT X tiles.  Shapes 6 and 7 are the encodings of a multires 15 / 6 model.
// cost: us per chunk and workgroup, every CU busy (tools/micro/dw_stamps.py), which is what dw_share_workgroups shares by.
// Every product streams the same number of chunks, but what a workgroup needs per chunk depends on the product's shape --
// bytes, MFMAs, and a cost per ring step that does not shrink with the chunk -- so sharing the workgroups by bytes let the
// narrow products finish last: at 196608 points the <8,2> product ended at 495 us and the head-alone one at 440 us when the
// 256 x 256 products were done at 385 us, and the launch takes as long as its last workgroup.
struct DwShape {
    int OT, IT, WO, WI;
    bool head;
    float cost_bf16, cost_split;
    size_t lds_bf16, lds_split;          // dynamic LDS of the body: ring slots x chunk image
};
constexpr int DW_SHAPES = 8;
constexpr DwShape DW_SHAPE[DW_SHAPES] = {
    {16, 16, 4, 2, false, 1.49f, 2.88f, dw_bf16_lds(16, 16, false), dw_split_lds(16, 16, false)},
    {8, 16, 4, 2, false, 1.06f, 1.91f, dw_bf16_lds(8, 16, false), dw_split_lds(8, 16, false)},
    {16, 4, 8, 1, false, 0.90f, 1.43f, dw_bf16_lds(16, 4, false), dw_split_lds(16, 4, false)},
    {8, 2, 8, 1, false, 0.56f, 0.80f, dw_bf16_lds(8, 2, false), dw_split_lds(8, 2, false)},
    {16, 16, 4, 2, true, 1.64f, 3.11f, dw_bf16_lds(16, 16, true), dw_split_lds(16, 16, true)},
    {0, 8, 0, 0, true, 0.43f, 0.544f, 12 * (9 * 1024), 7 * (18 * 1024)},       // dw_head_body / dw_head_split_body
    {16, 8, 4, 2, false, 1.06f, 1.91f, dw_bf16_lds(16, 8, false), dw_split_lds(16, 8, false)},
    {8, 4, 8, 1, false, 0.62f, 0.95f, dw_bf16_lds(8, 4, false), dw_split_lds(8, 4, false)},
};
constexpr size_t dw_lds_max() {
    size_t m = 0;
    for (int s = 0; s < DW_SHAPES; ++s) {
        if (DW_SHAPE[s].lds_bf16 > m) m = DW_SHAPE[s].lds_bf16;
        if (DW_SHAPE[s].lds_split > m) m = DW_SHAPE[s].lds_split;
    }
    return m;
}
constexpr size_t DW_LDS_MAX = dw_lds_max();      // what both kernels opt in to
static_assert(DW_LDS_MAX == 135168, "shape 4 in bf16: four ring slots of 32 KiB + 1 KiB");
constexpr bool dw_shape_is(int shape, int OT, int IT, int WO, int WI, bool head) {
    return DW_SHAPE[shape].OT == OT && DW_SHAPE[shape].IT == IT && DW_SHAPE[shape].WO == WO && DW_SHAPE[shape].WI == WI && DW_SHAPE[shape].head == head;
}

// The shape of a product with n_out_slots G columns and n_in_slots X columns, or -1.  Where only a row without head matches
// a product that has one, that row comes back: DwPlan::add refuses the head.
constexpr int dw_shape_of(int n_out_slots, int n_in_slots, bool head) {
    int found = -1;
    for (int s = 0; s < DW_SHAPES; ++s) {
        if (16 * DW_SHAPE[s].OT != n_out_slots || 16 * DW_SHAPE[s].IT != n_in_slots) continue;
        if (DW_SHAPE[s].head == head) return s;
        if (!DW_SHAPE[s].head) found = s;
    }
    return found;
}

// Workgroups per job: one each, then the next workgroup always goes to the job that would end last, up to cap per job and
// DW_GRID in all.
inline void dw_share_workgroups(const DwMulti &mj, bool split, int cap, int *nb) {
    int used = 0;
    for (int j = 0; j < mj.n; ++j) { nb[j] = 1; ++used; }
    for (; used < DW_GRID; ++used) {
        int best = -1;
        float worst = 0.f;
        for (int j = 0; j < mj.n; ++j) {
            const DwShape &sh = DW_SHAPE[mj.job[j].shape & 7];
            const float t = (split ? sh.cost_split : sh.cost_bf16) / (float)nb[j];
            if (nb[j] < cap && t > worst) { worst = t; best = j; }
        }
        if (best < 0) break;                                    // every product has as many workgroups as 8-chunk pieces
        ++nb[best];
    }
}

struct DwPlanes { const uint16_t *hi, *lo; };                   // a row array; lo (the plane of fp16 residuals) is NULL in bf16
// A head product (alpha_linear / rgb_linear): rows [row0, row0 + rows) of dL/draw's columns, H = kernels.h g_rawt.
struct DwHead {
    DwPlanes H;
    int row0, rows, ld;
    float *dW, *db;
};

struct DwPlan {
    DwMulti mj;
    DwReduceMulti mr;
    size_t lds = 0;                      // the largest LDS need among the jobs (layout)
    DwPlan() { mj.n = 0; mr.n = 0; }

    // One product: dW[:, col_off : col_off + m_valid] (+ db) of one Linear from G [P, n_out_slots] and X [P, n_in_slots];
    // with n_out_slots == 0 the head alone.  Every product overwrites its destination.
    int add(int64_t P, DwPlanes X, int n_in_slots, int in_kind, int in_L, int m_valid, DwPlanes G, int n_out_slots, int n_valid,
            float *dW, int ld_dw, int col_off, float *db, const DwHead *head, const float *inv_scale) {
        if (mj.n >= DW_MAX_JOBS) return NERF_AMD_EINVAL;
        const int shape = dw_shape_of(n_out_slots, n_in_slots, head != nullptr);
        if (shape < 0) return NERF_AMD_EUNSUPPORTED;
        if (head && !DW_SHAPE[shape].head) return NERF_AMD_EINVAL;      // a head rides on the 256 x 256 shape or stands alone
        DwJob &J = mj.job[mj.n];
        J.a.G = G.hi; J.a.G_lo = G.lo; J.a.ldg = n_out_slots; J.a.X = X.hi; J.a.X_lo = X.lo; J.a.ldx = n_in_slots; J.a.P = P;
        J.a.slab = nullptr; J.a.H = head ? head->H.hi : nullptr; J.a.H_lo = head ? head->H.lo : nullptr;
        J.shape = shape;
        J.first_block = 0; J.n_blocks = 0;
        DwReduceArgs &r = mr.r[mj.n];
        r.slab = nullptr; r.n_slabs = 0; r.OT = DW_SHAPE[shape].OT; r.IT = DW_SHAPE[shape].IT;
        r.dW = dW; r.ld_dw = ld_dw; r.col_off = col_off; r.db = db;
        r.out_kind = DW_SHAPE[shape].OT ? PERM_ACC : PERM_NAT; r.in_kind = in_kind; r.in_L = in_L; r.n_valid = n_valid; r.m_valid = m_valid;
        r.HT = head ? 1 : 0; r.head_dW = head ? head->dW : nullptr; r.head_db = head ? head->db : nullptr;
        r.head_row0 = head ? head->row0 : 0; r.head_rows = head ? head->rows : 0; r.head_ld = head ? head->ld : 0;
        r.inv_scale = inv_scale;
        ++mj.n;
        return NERF_AMD_OK;
    }

    // DW_GRID workgroups in all, shared by dw_share_workgroups (never more than a product has 8-chunk pieces); every
    // product's slabs follow the previous product's, and so do its reduction blocks.
    void layout(int64_t P, float *slab, bool split) {
        const int64_t n_chunks = (P + 31) / 32;
        int nb[DW_MAX_JOBS], per[DW_MAX_JOBS];
        for (int j = 0; j < mj.n; ++j) per[j] = dw_slab_floats(mr.r[j].OT, mr.r[j].IT, mr.r[j].HT);
        const int cap = n_chunks / 8 < 1 ? 1 : (int)(n_chunks / 8 > DW_GRID ? DW_GRID : n_chunks / 8);
        dw_share_workgroups(mj, split, cap, nb);
        float *sl = slab;
        int first = 0, rfirst = 0;
        lds = 0;
        for (int j = 0; j < mj.n; ++j) {
            mj.job[j].a.slab = sl;
            mj.job[j].first_block = first; mj.job[j].n_blocks = nb[j];
            mr.r[j].slab = sl; mr.r[j].n_slabs = nb[j];
            mr.first_block[j] = rfirst;
            sl += (size_t)nb[j] * per[j];
            first += nb[j];
            rfirst += (per[j] + DWR_BLOCK - 1) / DWR_BLOCK;
            const size_t need = split ? DW_SHAPE[mj.job[j].shape].lds_split : DW_SHAPE[mj.job[j].shape].lds_bf16;
            if (need > lds) lds = need;
        }
        mr.first_block[mj.n] = rfirst;
        mr.n = mj.n;
    }
    int n_blocks() const { return mj.n ? mj.job[mj.n - 1].first_block + mj.job[mj.n - 1].n_blocks : 0; }
    int n_reduce_blocks() const { return mr.first_block[mj.n]; }
};

}  // namespace na
