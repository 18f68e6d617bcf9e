// family_launch_check.cpp -- the GPU-free host logic of csrc/launch_util.h, run stand-alone (meant for a sanitizer build):
// the family table (for_family, family_known), pad_points and the group / deal arithmetic of launch_field (field_grid).
//
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip \
//         tools/family_launch_check.cpp -o family_launch_check && ./family_launch_check
//
// It calls no HIP function and needs no GPU.  It prints every result and exits 1 where one differs from the table below,
// which was written by hand from the launchers as they were before they shared launch_field:
//
// families (multires, views, view branch) -> <LX, LD, VD>; every other combination of {5,10,15} x {0,4,6} x {0,1} is unknown:
//   (10,4,1) -> <10,4,1>   (15,6,1) -> <15,6,1>   (10,*,0) -> <10,0,0>   (15,*,0) -> <15,0,0>     (views ignored without branch)
//
// launch arithmetic, 256-point tiles, n_cu = 256: groups = ceil(P / 256); a walking kernel (one workgroup per CU) caps the
// groups at n_cu and deals by ticket when groups > 2 * n_cu; P <= 0 launches nothing (OK), P >= 2^31 is EINVAL.
//   P              per-tile groups   walking groups   deal   pad_points
//   0              -  (OK, no launch)
//   1              1                 1                no     256
//   255            1                 1                no     256
//   256            1                 1                no     256
//   257            2                 2                no     512
//   131072         512               256              no     131072          (2 * 256 * n_cu: exactly two tiles each)
//   131073         513               256              yes    131328
//   2147483647     8388608           256              yes    2147483648
//   2147483648     -  (EINVAL)
#include <cstdio>

#include "../nerf_shared_amd/csrc/launch_util.h"

using namespace na;

static int bad = 0;
static void expect(bool ok, const char *what) {
    if (!ok) { std::printf("  MISMATCH: %s\n", what); ++bad; }
}

int main() {
    for (int mr : {5, 10, 15})
        for (int mv : {0, 4, 6})
            for (int vd : {0, 1}) {
                int lx = -1, ld = -1, fv = -1;
                const int rc = for_family(mr, mv, vd, [&](auto f) { lx = f.lx; ld = f.ld; fv = f.vd; return NERF_AMD_OK; });
                std::printf("family(%2d, %d, %d): rc %2d known %d -> <%d, %d, %d>\n", mr, mv, vd, rc, (int)family_known(mr, mv, vd), lx, ld, fv);
                const bool want = vd ? (mr == 10 && mv == 4) || (mr == 15 && mv == 6) : mr == 10 || mr == 15;
                expect(family_known(mr, mv, vd) == want && rc == (want ? NERF_AMD_OK : NERF_AMD_EUNSUPPORTED), "family coverage");
                if (want) expect(lx == mr && ld == (vd ? mv : 0) && fv == vd, "family tag");
                else expect(lx == -1, "callback ran for an unknown family");
            }
    expect(head_fits(true, 17) && head_fits(false, 16) && !head_fits(false, 17), "head_fits");

    const int64_t n_cu = 256;
    struct Row { int64_t P, per_tile, walking; bool deal; int64_t pad; };
    const Row rows[] = {{1, 1, 1, false, 256}, {255, 1, 1, false, 256}, {256, 1, 1, false, 256}, {257, 2, 2, false, 512},
                        {2 * 256 * n_cu, 512, 256, false, 131072}, {2 * 256 * n_cu + 1, 513, 256, true, 131328},
                        {((int64_t)1 << 31) - 1, 8388608, 256, true, (int64_t)1 << 31}};
    for (const int64_t P : {(int64_t)0, (int64_t)1 << 31})
        std::printf("P %10lld: %lld groups, never launched: launch_field returns %s first\n", (long long)P,
                    (long long)field_grid(P, 256, n_cu, true).groups, P <= 0 ? "OK" : "EINVAL");
    for (const Row &r : rows) {
        const FieldGrid tile = field_grid(r.P, 256, 0, true), walk = field_grid(r.P, 256, n_cu, true), off = field_grid(r.P, 256, n_cu, false);
        std::printf("P %10lld: per tile %lld groups; walking %lld groups, deal %d (tickets off: %d); pad_points %lld\n", (long long)r.P,
                    (long long)tile.groups, (long long)walk.groups, (int)walk.deal, (int)off.deal, (long long)pad_points(r.P));
        expect(tile.groups == r.per_tile && !tile.deal, "per-tile grid");
        expect(walk.groups == r.walking && walk.deal == r.deal, "walking grid");
        expect(off.groups == r.walking && !off.deal, "walking grid, tickets off (A/B 42)");
        expect(pad_points(r.P) == r.pad, "pad_points");
    }
    std::printf(bad ? "%d MISMATCHES\n" : "all as expected\n", bad);
    return bad ? 1 : 0;
}
