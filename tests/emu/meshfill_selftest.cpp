// meshfill_selftest.cpp -- a stand-alone program over the host twin of csrc/meshfill_core.h (link with meshfill_emu.cpp and
// meshtopo_emu.cpp): a tetrahedron and a cube with a hole, an open cone of 129 rim vertices in both modes and both walking
// orders, a bow-tie and the error paths.  Meant to be built with -fsanitize=address,undefined as well (DESIGN.md section 4j
// gives the line): it exercises the compaction, both doublings, the scans and the emit on the host.
#include <stdint.h>
#include <stdio.h>

#include <vector>

extern "C" {
int r3g_emu_meshfill_plan(const float* v, int64_t nv, const int32_t* f, int64_t nf, int64_t max_loop, int mode, int reverse,
                          int64_t* report);
int r3g_emu_meshfill_emit(int32_t* new_faces, float* new_verts);
int r3g_emu_meshfill_loops(int64_t* loop_start, int32_t* loop_verts, int32_t* status);
int r3g_emu_meshtopo_build(const float* v, int64_t nv, const int32_t* f, int64_t nf, int reverse, int32_t* mate, int32_t* body,
                           uint8_t* flip, int64_t* report, int* rounds_out);
}

#define CHECK(x)                                              \
    do {                                                      \
        if (!(x)) {                                           \
            printf("meshfill selftest FAILED: %s\n", #x);     \
            return 1;                                         \
        }                                                     \
    } while (0)

// report fields: 0 boundary, 1 loops, 2 tangled, 3 filled, 4 oversize, 5 longest, 6 loop_edges, 7 faces_added, 8 verts_added, 9 rounds
int main() {
    int64_t rep[16], topo[16];
    CHECK(r3g_emu_meshfill_emit(nullptr, nullptr) == -3);                      // no plan yet

    // a tetrahedron without its last face (0, 3, 2)
    const float tv[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    const int32_t tf[9] = {0, 2, 1, 0, 1, 3, 1, 2, 3};
    CHECK(r3g_emu_meshfill_plan(tv, 4, tf, 3, 64, 0, 0, rep) == 0);
    CHECK(rep[0] == 3 && rep[1] == 1 && rep[2] == 0 && rep[3] == 1 && rep[5] == 3 && rep[7] == 1 && rep[8] == 0 && rep[9] == 2);
    int32_t nf3[3];
    CHECK(r3g_emu_meshfill_emit(nf3, nullptr) == 0);
    CHECK((nf3[0] == 0 && nf3[1] == 3 && nf3[2] == 2) || (nf3[0] == 3 && nf3[1] == 2 && nf3[2] == 0) || (nf3[0] == 2 && nf3[1] == 0 && nf3[2] == 3));

    // the unit cube (vertex 4 x + 2 y + z) without the side z = 1
    std::vector<float> cv;
    for (int x = 0; x < 2; ++x)
        for (int y = 0; y < 2; ++y)
            for (int z = 0; z < 2; ++z) cv.insert(cv.end(), {(float)x, (float)y, (float)z});
    const int quads[5][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}};
    std::vector<int32_t> cube;
    for (auto& q : quads) cube.insert(cube.end(), {q[0], q[1], q[2], q[0], q[2], q[3]});
    CHECK(r3g_emu_meshfill_plan(cv.data(), 8, cube.data(), 10, 64, 1, 0, rep) == 0);
    CHECK(rep[0] == 4 && rep[1] == 1 && rep[3] == 1 && rep[5] == 4 && rep[7] == 4 && rep[8] == 1);
    std::vector<int32_t> added(12);
    float centre[3];
    CHECK(r3g_emu_meshfill_emit(added.data(), centre) == 0);
    CHECK(centre[0] == 0.5f && centre[1] == 0.5f && centre[2] == 1.0f);
    cube.insert(cube.end(), added.begin(), added.end());
    cv.insert(cv.end(), centre, centre + 3);
    CHECK(r3g_emu_meshtopo_build(cv.data(), 9, cube.data(), 14, 0, nullptr, nullptr, nullptr, topo, nullptr) == 0);
    CHECK(topo[4] == 0 && topo[5] == 0 && topo[6] == 0 && topo[9] == 2 && topo[11] == (6ll << topo[12]));
    CHECK(r3g_emu_meshfill_plan(cv.data(), 9, cube.data(), 14, 64, 0, 0, rep) == 0 && rep[0] == 0 && rep[7] == 0 && rep[9] == 0);
    CHECK(r3g_emu_meshfill_plan(cv.data(), 9, cube.data(), 10, 3, 0, 0, rep) == 0 && rep[4] == 1 && rep[3] == 0 && rep[7] == 0);

    // an open cone: apex 0, rim 1 .. n
    const int n = 129;
    std::vector<float> kv(3 * (n + 1), 0.0f);
    kv[2] = 1.0f;
    for (int i = 0; i < n; ++i) kv[3 * (i + 1)] = (float)(i % 7), kv[3 * (i + 1) + 1] = (float)(i % 5);
    std::vector<int32_t> kf;
    for (int i = 0; i < n; ++i) kf.insert(kf.end(), {0, 1 + i, 1 + (i + 1) % n});
    for (int mode = 0; mode < 2; ++mode)
        for (int reverse = 0; reverse < 2; ++reverse) {
            CHECK(r3g_emu_meshfill_plan(kv.data(), n + 1, kf.data(), n, n, mode, reverse, rep) == 0);
            CHECK(rep[0] == n && rep[1] == 1 && rep[2] == 0 && rep[3] == 1 && rep[5] == n && rep[6] == n && rep[9] == 8);
            CHECK(rep[7] == (mode ? n : n - 2) && rep[8] == mode);
            std::vector<int64_t> start(2);
            std::vector<int32_t> lv(n), status(1), faces(3 * rep[7]);
            std::vector<float> nv(3 * rep[8] + 1);
            CHECK(r3g_emu_meshfill_loops(start.data(), lv.data(), status.data()) == 0);
            CHECK(start[0] == 0 && start[1] == n && status[0] == 0);
            // half-edge 1 = (1 -> 2) leads; the boundary runs 1, 2, ..., n
            for (int i = 0; i < n; ++i) CHECK(lv[i] == 1 + i);
            CHECK(r3g_emu_meshfill_emit(faces.data(), nv.data()) == 0);
            std::vector<int32_t> all = kf;
            all.insert(all.end(), faces.begin(), faces.end());
            CHECK(r3g_emu_meshtopo_build(nullptr, n + 1 + mode, all.data(), (int64_t)all.size() / 3, 0, nullptr, nullptr, nullptr, topo, nullptr) == 0);
            CHECK(topo[4] == 0 && topo[5] == 0 && topo[6] == 0 && topo[9] == 2);
            CHECK(r3g_emu_meshfill_plan(kv.data(), n + 1, kf.data(), n, n - 1, mode, reverse, rep) == 0 && rep[4] == 1 && rep[7] == 0);
        }

    // a bow-tie: two open fans of three faces around apexes 0 and 5 whose rims meet in vertex 1 -- every boundary half-edge
    // lies on a chain through the pinch
    const int32_t bf[] = {0, 1, 2, 0, 2, 3, 0, 3, 1, 5, 1, 6, 5, 6, 7, 5, 7, 1};
    CHECK(r3g_emu_meshfill_plan(nullptr, 8, bf, 6, 64, 0, 0, rep) == 0);
    CHECK(rep[0] == 6 && rep[1] == 0 && rep[2] == 6 && rep[7] == 0);

    // errors: bad index, max_loop, mode, centroid without vertices, no face; a failed plan leaves no state
    int32_t bad[9] = {0, 2, 1, 0, 1, 4, 1, 2, 3};
    CHECK(r3g_emu_meshfill_plan(tv, 4, bad, 3, 64, 0, 0, rep) == -2);
    CHECK(r3g_emu_meshfill_emit(nullptr, nullptr) == -3);
    CHECK(r3g_emu_meshfill_plan(tv, 4, tf, 3, 2, 0, 0, rep) == -1);
    CHECK(r3g_emu_meshfill_plan(tv, 4, tf, 3, 64, 2, 0, rep) == -1);
    CHECK(r3g_emu_meshfill_plan(nullptr, 4, tf, 3, 64, 1, 0, rep) == -1);
    CHECK(r3g_emu_meshfill_plan(tv, 4, tf, 0, 64, 0, 0, rep) == -1);
    printf("meshfill selftest ok\n");
    return 0;
}
