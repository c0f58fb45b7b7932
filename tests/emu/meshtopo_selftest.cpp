// meshtopo_selftest.cpp -- a stand-alone program over the host twin of csrc/meshtopo_core.h (link with meshtopo_emu.cpp): the
// unit cube with one face reversed and a Moebius strip through build and orient.  Meant to be built with
// -fsanitize=address,undefined as well: it exercises the edge table, the label rounds and the sums on the host.
#include <stdint.h>
#include <stdio.h>

#include <vector>

extern "C" {
int r3g_emu_meshtopo_build(const float* v, int64_t nv, const int32_t* f, int64_t nf, int reverse, int32_t* mate, int32_t* body,
                           uint8_t* flip, int64_t* report, int* rounds_out);
int r3g_emu_meshtopo_orient(const float* v, int64_t nv, int32_t* f, int64_t nf, int outward, int reverse, int64_t* faces_reversed,
                            int64_t* bodies_reversed, int32_t* mate, int32_t* body, uint8_t* flip, int64_t* report);
}

#define CHECK(x)                                              \
    do {                                                      \
        if (!(x)) {                                           \
            printf("meshtopo selftest FAILED: %s\n", #x);     \
            return 1;                                         \
        }                                                     \
    } while (0)

int main() {
    // the unit cube, vertex 4 x + 2 y + z, wound outward
    std::vector<float> cv;
    for (int x = 0; x < 2; ++x)
        for (int y = 0; y < 2; ++y)
            for (int z = 0; z < 2; ++z) cv.insert(cv.end(), {(float)x, (float)y, (float)z});
    const int quads[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};
    std::vector<int32_t> cube;
    for (auto& q : quads) cube.insert(cube.end(), {q[0], q[1], q[2], q[0], q[2], q[3]});
    std::vector<int32_t> mate(36), body(12);
    std::vector<uint8_t> flip(12);
    int64_t rep[16];
    int rounds = 0;
    for (int reverse = 0; reverse < 2; ++reverse) {
        CHECK(r3g_emu_meshtopo_build(cv.data(), 8, cube.data(), 12, reverse, mate.data(), body.data(), flip.data(), rep, &rounds) == 0);
        CHECK(rep[0] == 12 && rep[2] == 8 && rep[3] == 18 && rep[9] == 2 && rep[4] == 0 && rep[5] == 0 && rep[6] == 0 && rep[7] == 1);
        CHECK(rep[11] == (6ll << rep[12]) && rep[13] == (12ll << rep[14]) && rounds > 0);
    }
    std::vector<int32_t> bent = cube;
    bent[3 * 5] = cube[3 * 5 + 2], bent[3 * 5 + 2] = cube[3 * 5];
    int64_t nfr = 0, nbr = 0;
    CHECK(r3g_emu_meshtopo_orient(cv.data(), 8, bent.data(), 12, 2, 0, &nfr, &nbr, mate.data(), body.data(), flip.data(), rep) == 0);
    CHECK(nfr == 1 && nbr == 0 && bent == cube && rep[5] == 0);
    std::vector<int32_t> inward = cube;
    for (int f = 0; f < 12; ++f) inward[3 * f] = cube[3 * f + 2], inward[3 * f + 2] = cube[3 * f];
    CHECK(r3g_emu_meshtopo_orient(cv.data(), 8, inward.data(), 12, 1, 1, &nfr, &nbr, nullptr, nullptr, nullptr, rep) == 0);
    CHECK(nfr == 12 && nbr == 1 && inward == cube && rep[11] > 0);
    bent[0] = 8;
    CHECK(r3g_emu_meshtopo_build(cv.data(), 8, bent.data(), 12, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == -2);

    // a Moebius strip of n quads: top i, bottom n + i; the seam joins top to bottom
    const int n = 8;
    std::vector<float> mv(6 * n, 0.0f);
    for (int i = 0; i < 2 * n; ++i) mv[3 * i] = (float)(i % n), mv[3 * i + 1] = (float)(i / n);
    std::vector<int32_t> mf;
    for (int i = 0; i < n; ++i) {
        const int t0 = i, b0 = n + i, t1 = i + 1 < n ? i + 1 : n, b1 = i + 1 < n ? n + i + 1 : 0;
        mf.insert(mf.end(), {t0, b0, t1, b0, b1, t1});
    }
    const std::vector<int32_t> before = mf;
    mate.resize(6 * n), body.resize(2 * n), flip.resize(2 * n);
    for (int outward = 0; outward < 3; ++outward) {
        CHECK(r3g_emu_meshtopo_orient(mv.data(), 2 * n, mf.data(), 2 * n, outward, 0, &nfr, &nbr, mate.data(), body.data(), flip.data(), rep) == 0);
        CHECK(nfr == 0 && nbr == 0 && mf == before && rep[7] == 1 && rep[8] == 1 && rep[4] == 2 * n);
        for (int f = 0; f < 2 * n; ++f) CHECK(body[f] == 0 && flip[f] == 0);
    }
    printf("meshtopo selftest ok\n");
    return 0;
}
