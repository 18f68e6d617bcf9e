// dw_plan_check.cpp -- the GPU-free host logic of csrc/dw_plan.h, run stand-alone (meant for a sanitizer build): the table of
// job shapes (dw_shape_of), the plan of every model family in both precisions (DwPlan::add, DwPlan::layout with
// dw_share_workgroups) and the error returns of add.
//
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip \
//         tools/dw_plan_check.cpp -o dw_plan_check && ./dw_plan_check
//
// It calls no HIP function and needs no GPU.  It prints every plan and exits 1 where something differs from the literals
// below.  They are what the launchers computed before they shared the planner (commit 00b8d5d: DwSeq::flush for bf16,
// train_param_grads_split for split precision), printed by a copy of that code; first blocks and slab offsets are checked
// as running sums of the literal workgroup counts and the literal slab sizes per shape.
//
// Jobs in launch order: layer 0, layers 1-4, the skip layer's two products, layers 6-7, and with a view branch
// feature_linear + alpha head, views_linears.0 over the feature, over the directions, and the rgb head alone.
// Point counts: 1, 480 | 481 (at most n_chunks / 8 workgroups per job: 1 -> 2), 5633 and 7500 (the cap, 22 and 29, gives way
// to the cost table), 65536 and 196608 (a 1024-ray step's coarse and fine pass), 8388352 = 2^23 - 256 (the split limit).
#include <cstdio>

#include "../nerf_shared_amd/csrc/dw_plan.h"

using namespace na;

static int bad = 0;
static void expect(bool ok, const char *what) {
    if (!ok) { std::printf("  MISMATCH: %s\n", what); ++bad; }
}

// per shape id: slab floats of one workgroup, LDS bytes of the bf16 and of the split body
static const int SLAB[8] = {65792, 32896, 16640, 4224, 69904, 2064, 33024, 8320};
static const size_t LDS_BF16[8] = {131072, 122880, 122880, 122880, 135168, 110592, 122880, 122880};
static const size_t LDS_SPLIT[8] = {131072, 98304, 122880, 122880, 135168, 129024, 98304, 122880};

struct Family { const char *name; int E, Dd; bool view; int n; int shape[13]; int reduce_first[14]; };
static const Family FAMILY[4] = {
    {"(10,4,view)", 64, 32, true, 13, {2, 0, 0, 0, 0, 2, 0, 0, 0, 4, 1, 3, 5}, {0, 33, 162, 291, 420, 549, 582, 711, 840, 969, 1106, 1171, 1180, 1185}},
    {"(15,6,view)", 128, 64, true, 13, {6, 0, 0, 0, 0, 6, 0, 0, 0, 4, 1, 7, 5}, {0, 65, 194, 323, 452, 581, 646, 775, 904, 1033, 1170, 1235, 1252, 1257}},
    {"(10,.,no view)", 64, 0, false, 9, {2, 0, 0, 0, 0, 2, 0, 0, 0}, {0, 33, 162, 291, 420, 549, 582, 711, 840, 969}},
    {"(15,.,no view)", 128, 0, false, 9, {6, 0, 0, 0, 0, 6, 0, 0, 0}, {0, 65, 194, 323, 452, 581, 646, 775, 904, 1033}},
};
struct Case { int family, split; long long P; int nb[13]; int grid; long long slab_end; size_t lds; };
static const Case CASES[] = {
    {0, 0, 1, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, 13, 602912, 135168},
    {0, 0, 480, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, 13, 602912, 135168},
    {0, 0, 481, {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2}, 26, 1205824, 135168},
    {0, 0, 5633, {19, 22, 22, 22, 22, 18, 22, 22, 22, 22, 22, 12, 9}, 256, 13078512, 135168},
    {0, 0, 7500, {15, 24, 24, 24, 24, 14, 24, 24, 24, 26, 17, 9, 7}, 256, 13964816, 135168},
    {0, 0, 65536, {15, 24, 24, 24, 24, 14, 24, 24, 24, 26, 17, 9, 7}, 256, 13964816, 135168},
    {0, 0, 196608, {15, 24, 24, 24, 24, 14, 24, 24, 24, 26, 17, 9, 7}, 256, 13964816, 135168},
    {0, 0, 8388352, {15, 24, 24, 24, 24, 14, 24, 24, 24, 26, 17, 9, 7}, 256, 13964816, 135168},
    {0, 1, 1, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, 13, 602912, 135168},
    {0, 1, 480, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, 13, 602912, 135168},
    {0, 1, 481, {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2}, 26, 1205824, 135168},
    {0, 1, 5633, {20, 22, 22, 22, 22, 19, 22, 22, 22, 22, 22, 11, 8}, 256, 13105504, 135168},
    {0, 1, 7500, {13, 25, 25, 25, 25, 12, 25, 25, 25, 27, 17, 7, 5}, 256, 14416128, 135168},
    {0, 1, 65536, {13, 25, 25, 25, 25, 12, 25, 25, 25, 27, 17, 7, 5}, 256, 14416128, 135168},
    {0, 1, 196608, {13, 25, 25, 25, 25, 12, 25, 25, 25, 27, 17, 7, 5}, 256, 14416128, 135168},
    {0, 1, 8388352, {13, 25, 25, 25, 25, 12, 25, 25, 25, 27, 17, 7, 5}, 256, 14416128, 135168},
    {1, 0, 1, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, 13, 639776, 135168},
    {1, 0, 480, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, 13, 639776, 135168},
    {1, 0, 481, {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2}, 26, 1279552, 135168},
    {1, 0, 5633, {20, 22, 22, 22, 22, 20, 22, 22, 22, 22, 20, 12, 8}, 256, 13765088, 135168},
    {1, 0, 7500, {17, 24, 23, 23, 23, 17, 23, 23, 23, 26, 17, 10, 7}, 256, 14255504, 135168},
    {1, 0, 65536, {17, 24, 23, 23, 23, 17, 23, 23, 23, 26, 17, 10, 7}, 256, 14255504, 135168},
    {1, 0, 196608, {17, 24, 23, 23, 23, 17, 23, 23, 23, 26, 17, 10, 7}, 256, 14255504, 135168},
    {1, 0, 8388352, {17, 24, 23, 23, 23, 17, 23, 23, 23, 26, 17, 10, 7}, 256, 14255504, 135168},
    {1, 1, 1, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, 13, 639776, 135168},
    {1, 1, 480, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, 13, 639776, 135168},
    {1, 1, 481, {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2}, 26, 1279552, 135168},
    {1, 1, 5633, {21, 22, 22, 22, 22, 21, 22, 22, 22, 22, 21, 11, 6}, 256, 13851584, 135168},
    {1, 1, 7500, {16, 25, 24, 24, 24, 16, 24, 24, 24, 26, 16, 8, 5}, 256, 14596336, 135168},
    {1, 1, 65536, {16, 25, 24, 24, 24, 16, 24, 24, 24, 26, 16, 8, 5}, 256, 14596336, 135168},
    {1, 1, 196608, {16, 25, 24, 24, 24, 16, 24, 24, 24, 26, 16, 8, 5}, 256, 14596336, 135168},
    {1, 1, 8388352, {16, 25, 24, 24, 24, 16, 24, 24, 24, 26, 16, 8, 5}, 256, 14596336, 135168},
    {2, 0, 1, {1, 1, 1, 1, 1, 1, 1, 1, 1}, 9, 493824, 135168},
    {2, 0, 480, {1, 1, 1, 1, 1, 1, 1, 1, 1}, 9, 493824, 135168},
    {2, 0, 481, {2, 2, 2, 2, 2, 2, 2, 2, 2}, 18, 987648, 135168},
    {2, 0, 5633, {22, 22, 22, 22, 22, 22, 22, 22, 22}, 198, 10864128, 135168},
    {2, 0, 7500, {27, 29, 29, 29, 29, 26, 29, 29, 29}, 256, 14237696, 135168},
    {2, 0, 65536, {19, 32, 31, 31, 31, 19, 31, 31, 31}, 256, 14974976, 135168},
    {2, 0, 196608, {19, 32, 31, 31, 31, 19, 31, 31, 31}, 256, 14974976, 135168},
    {2, 0, 8388352, {19, 32, 31, 31, 31, 19, 31, 31, 31}, 256, 14974976, 135168},
    {2, 1, 1, {1, 1, 1, 1, 1, 1, 1, 1, 1}, 9, 493824, 131072},
    {2, 1, 480, {1, 1, 1, 1, 1, 1, 1, 1, 1}, 9, 493824, 131072},
    {2, 1, 481, {2, 2, 2, 2, 2, 2, 2, 2, 2}, 18, 987648, 131072},
    {2, 1, 5633, {22, 22, 22, 22, 22, 22, 22, 22, 22}, 198, 10864128, 131072},
    {2, 1, 7500, {27, 29, 29, 29, 29, 26, 29, 29, 29}, 256, 14237696, 131072},
    {2, 1, 65536, {16, 32, 32, 32, 32, 16, 32, 32, 32}, 256, 15269888, 131072},
    {2, 1, 196608, {16, 32, 32, 32, 32, 16, 32, 32, 32}, 256, 15269888, 131072},
    {2, 1, 8388352, {16, 32, 32, 32, 32, 16, 32, 32, 32}, 256, 15269888, 131072},
    {3, 0, 1, {1, 1, 1, 1, 1, 1, 1, 1, 1}, 9, 526592, 135168},
    {3, 0, 480, {1, 1, 1, 1, 1, 1, 1, 1, 1}, 9, 526592, 135168},
    {3, 0, 481, {2, 2, 2, 2, 2, 2, 2, 2, 2}, 18, 1053184, 135168},
    {3, 0, 5633, {22, 22, 22, 22, 22, 22, 22, 22, 22}, 198, 11585024, 135168},
    {3, 0, 7500, {27, 29, 29, 29, 29, 26, 29, 29, 29}, 256, 15106048, 135168},
    {3, 0, 65536, {22, 31, 31, 30, 30, 22, 30, 30, 30}, 256, 15400960, 135168},
    {3, 0, 196608, {22, 31, 31, 30, 30, 22, 30, 30, 30}, 256, 15400960, 135168},
    {3, 0, 8388352, {22, 31, 31, 30, 30, 22, 30, 30, 30}, 256, 15400960, 135168},
    {3, 1, 1, {1, 1, 1, 1, 1, 1, 1, 1, 1}, 9, 526592, 131072},
    {3, 1, 480, {1, 1, 1, 1, 1, 1, 1, 1, 1}, 9, 526592, 131072},
    {3, 1, 481, {2, 2, 2, 2, 2, 2, 2, 2, 2}, 18, 1053184, 131072},
    {3, 1, 5633, {22, 22, 22, 22, 22, 22, 22, 22, 22}, 198, 11585024, 131072},
    {3, 1, 7500, {27, 29, 29, 29, 29, 26, 29, 29, 29}, 256, 15106048, 131072},
    {3, 1, 65536, {20, 31, 31, 31, 31, 20, 31, 31, 30}, 256, 15532032, 131072},
    {3, 1, 196608, {20, 31, 31, 31, 31, 20, 31, 31, 30}, 256, 15532032, 131072},
    {3, 1, 8388352, {20, 31, 31, 31, 31, 20, 31, 31, 30}, 256, 15532032, 131072},
};

static uint16_t dummy_rows[8];      // stands for every row array: the planner never reads through the pointers
static float dummy_out[8];
static float dummy_slab[256 * (256 * 256 + 256)];       // the half of the slab buffer that the jobs of a plan share (backward.hip SLAB_FLOATS)

// The products of a family, as backward.hip's layer walk adds them (W = 256, D = 8, skip after layer 4).
static int add_family(DwPlan &plan, const Family &f, int64_t P, bool split) {
    const DwPlanes R{dummy_rows, split ? dummy_rows : nullptr}, none{nullptr, nullptr};
    const float *inv = split ? dummy_out : nullptr;
    const int W = 256;
    int rc = NERF_AMD_OK;
    auto product = [&](int n_in_slots, int in_kind, DwPlanes G, int n_out_slots, const DwHead *head = nullptr) {
        if (!rc) rc = plan.add(P, R, n_in_slots, in_kind, 0, n_in_slots, G, n_out_slots, n_out_slots, dummy_out, W, 0, dummy_out, head, inv);
    };
    for (int l = 0; l < 8; ++l) {
        if (l == 0 || l == 5) product(f.E, PERM_GEN, R, W);
        if (l != 0) product(W, PERM_ACC, R, W);
    }
    if (f.view) {
        const DwHead alpha{R, 3, 1, W, dummy_out, dummy_out}, rgb{R, 0, 3, W / 2, dummy_out, dummy_out};
        product(W, PERM_ACC, R, W, &alpha);
        product(W, PERM_ACC, R, W / 2);
        product(f.Dd, PERM_GEN, R, W / 2);
        product(W / 2, PERM_ACC, none, 0, &rgb);
    }
    return rc;
}

int main() {
    // ---- the shape table
    struct ShapeRow { int n_out, n_in; bool head; int want; };
    const ShapeRow shape_rows[] = {{256, 256, false, 0}, {128, 256, false, 1}, {256, 64, false, 2}, {128, 32, false, 3}, {256, 256, true, 4},
                                   {0, 128, true, 5}, {256, 128, false, 6}, {128, 64, false, 7},
                                   // outside the table
                                   {0, 128, false, -1}, {0, 256, true, -1}, {256, 32, false, -1}, {128, 128, false, -1}, {64, 256, false, -1},
                                   {256, 96, false, -1}, {250, 256, false, -1}, {256, 0, false, -1},
                                   // a head on a shape that carries none: the shape itself (add refuses the head)
                                   {128, 256, true, 1}, {256, 64, true, 2}, {128, 32, true, 3}, {256, 128, true, 6}, {128, 64, true, 7}};
    for (const ShapeRow &r : shape_rows) {
        const int got = dw_shape_of(r.n_out, r.n_in, r.head);
        std::printf("dw_shape_of(%3d, %3d, %d) = %2d\n", r.n_out, r.n_in, (int)r.head, got);
        expect(got == r.want, "dw_shape_of");
    }
    const int OTs[8] = {16, 8, 16, 8, 16, 0, 16, 8}, ITs[8] = {16, 16, 4, 2, 16, 8, 8, 4};
    for (int s = 0; s < 8; ++s) {
        std::printf("shape %d: <%2d, %2d, %d, %d, %d>  slab %5d floats  LDS %6zu bf16 %6zu split\n", s, DW_SHAPE[s].OT, DW_SHAPE[s].IT, DW_SHAPE[s].WO,
                    DW_SHAPE[s].WI, (int)DW_SHAPE[s].head, dw_slab_floats(DW_SHAPE[s].OT, DW_SHAPE[s].IT, DW_SHAPE[s].head), DW_SHAPE[s].lds_bf16,
                    DW_SHAPE[s].lds_split);
        expect(DW_SHAPE[s].OT == OTs[s] && DW_SHAPE[s].IT == ITs[s] && DW_SHAPE[s].head == (s == 4 || s == 5), "shape row");
        expect(dw_slab_floats(DW_SHAPE[s].OT, DW_SHAPE[s].IT, DW_SHAPE[s].head) == SLAB[s], "slab floats of a shape");
        expect(DW_SHAPE[s].lds_bf16 == LDS_BF16[s] && DW_SHAPE[s].lds_split == LDS_SPLIT[s], "LDS bytes of a shape");
    }
    expect(DW_LDS_MAX == 135168 && DW_GRID == 256 && DW_MAX_JOBS == 16 && DWR_BLOCK == 512, "constants");

    // ---- the plans
    for (const Case &c : CASES) {
        const Family &f = FAMILY[c.family];
        DwPlan plan;
        const int rc = add_family(plan, f, c.P, c.split != 0);
        plan.layout(c.P, dummy_slab, c.split != 0);
        std::printf("%-15s %-5s P %7lld: rc %d, %2d jobs, grid %3d, %4d reduce blocks, slabs end at %8lld, LDS %zu (launched with %zu); nb",
                    f.name, c.split ? "split" : "bf16", c.P, rc, plan.mj.n, plan.n_blocks(), plan.n_reduce_blocks(),
                    plan.mj.n ? (long long)(plan.mj.job[plan.mj.n - 1].a.slab - dummy_slab) + (long long)plan.mj.job[plan.mj.n - 1].n_blocks * SLAB[plan.mj.job[plan.mj.n - 1].shape & 7] : 0LL,
                    plan.lds, c.split ? plan.lds : DW_LDS_MAX);
        for (int j = 0; j < plan.mj.n; ++j) std::printf(" %d", plan.mj.job[j].n_blocks);
        std::printf("\n");
        expect(rc == NERF_AMD_OK && plan.mj.n == f.n && plan.mr.n == f.n, "number of jobs");
        if (plan.mj.n != f.n) continue;
        int first = 0;
        long long off = 0;
        for (int j = 0; j < f.n; ++j) {
            const DwJob &J = plan.mj.job[j];
            const DwReduceArgs &r = plan.mr.r[j];
            expect(J.shape == f.shape[j], "shape id");
            expect(J.n_blocks == c.nb[j] && r.n_slabs == c.nb[j], "nb[]");
            expect(J.first_block == first, "first_block[]");
            expect(J.a.slab - dummy_slab == off && r.slab == J.a.slab, "slab offset");
            expect(plan.mr.first_block[j] == f.reduce_first[j], "reduce first block");
            expect(J.a.P == c.P && (J.a.X_lo != nullptr) == (c.split != 0) && (r.inv_scale != nullptr) == (c.split != 0), "precision of a job");
            expect(r.OT == OTs[f.shape[j]] && r.IT == ITs[f.shape[j]] && r.HT == (f.shape[j] == 4 || f.shape[j] == 5), "reduce tiles");
            expect(r.out_kind == (f.shape[j] == 5 ? PERM_NAT : PERM_ACC), "out_kind");
            first += c.nb[j];
            off += (long long)c.nb[j] * SLAB[f.shape[j]];
        }
        expect(plan.mr.first_block[f.n] == f.reduce_first[f.n] && plan.n_reduce_blocks() == f.reduce_first[f.n], "reduce blocks");
        expect(plan.n_blocks() == c.grid && first == c.grid, "grid");
        expect(off == c.slab_end && off <= (long long)(sizeof(dummy_slab) / sizeof(float)), "end of the slabs");
        // bf16 launches with DW_LDS_MAX whatever the jobs need; split with the largest need among its jobs
        expect((c.split ? plan.lds : DW_LDS_MAX) == c.lds && plan.lds <= DW_LDS_MAX, "LDS request");
    }

    // ---- error returns of add
    {
        const DwPlanes R{dummy_rows, nullptr};
        const DwHead head{R, 0, 1, 256, dummy_out, dummy_out};
        auto add = [&](DwPlan &p, int n_in, int n_out, const DwHead *h) {
            return p.add(1024, R, n_in, PERM_ACC, 0, n_in, R, n_out, n_out, dummy_out, 256, 0, dummy_out, h, nullptr);
        };
        DwPlan p;
        expect(add(p, 96, 256, nullptr) == NERF_AMD_EUNSUPPORTED && add(p, 128, 0, nullptr) == NERF_AMD_EUNSUPPORTED, "a shape outside the table");
        expect(add(p, 256, 128, &head) == NERF_AMD_EINVAL && add(p, 64, 256, &head) == NERF_AMD_EINVAL, "a head on a shape other than 4 and 5");
        expect(p.mj.n == 0, "a refused product leaves no job");
        expect(add(p, 256, 256, &head) == NERF_AMD_OK && p.mj.job[0].shape == 4 && add(p, 128, 0, &head) == NERF_AMD_OK && p.mj.job[1].shape == 5, "heads on shapes 4 and 5");
        for (int j = 2; j < DW_MAX_JOBS; ++j) expect(add(p, 256, 256, nullptr) == NERF_AMD_OK, "up to DW_MAX_JOBS jobs");
        expect(p.mj.n == DW_MAX_JOBS && add(p, 256, 256, nullptr) == NERF_AMD_EINVAL && p.mj.n == DW_MAX_JOBS, "more than DW_MAX_JOBS jobs");
        std::printf("add: errors checked\n");
    }
    std::printf(bad ? "%d MISMATCHES\n" : "all as expected\n", bad);
    return bad ? 1 : 0;
}
