// standoff_walk_main.cpp -- the nearest-distance walk of the fleet loop's stand-off term (bluerov2_amd/csrc/standoff_walk.hpp) on the host
// alone, for tests/test_standoff_cpu.py, which compiles this file with -ffp-contract=off -fsanitize=address,undefined and runs it directly.
// Arguments: <triangles> <points> <out> <reach>: files of raw float64 triangles [T][3][3] and points [P][3], the file to write, and a
// finite reach.  For every leaf size 1 ... 8 and for reach2 = reach * reach and +Inf it builds the hierarchy (mesh_bvh.hpp) and checks, for
// every point without a NaN coordinate (the callers of the walk skip the others: their value is reach2), that
//   - the walk started at reach2 returns the bytes of testing every triangle, started at reach2
//   - the walk with the finite reach makes no more node tests and no more triangle tests than the walk with +Inf
// and prints "leaf <l> reach <r> => ok node_tests <mean> tri_tests <mean>" or the first failure.  <out> receives [2][P] doubles: the values
// for the finite reach, then those for +Inf (the same for every leaf size, or the run has failed).  Exit code 1 on a failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "standoff_walk.hpp"

using namespace brov;

static bool read_doubles(const char* path, std::vector<double>& v) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    double buf[512];
    size_t n;
    while ((n = std::fread(buf, sizeof(double), 512, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 5) { std::printf("usage: %s triangles points out reach\n", argv[0]); return 2; }
    std::vector<double> tri, pts;
    if (!read_doubles(argv[1], tri) || !read_doubles(argv[2], pts) || tri.size() % 9 || pts.size() % 3 || tri.empty()) {
        std::printf("cannot read %s or %s\n", argv[1], argv[2]);
        return 2;
    }
    const double reach = std::atof(argv[4]);
    const int64_t T = (int64_t)tri.size() / 9, P = (int64_t)pts.size() / 3;
    const double seeds[2] = {reach * reach, HUGE_VAL};
    std::vector<double> out((size_t)(2 * P)), first((size_t)(2 * P));
    int bad = 0;
    for (int leaf = 1; leaf <= 8; leaf++) {
        MeshBvh h;
        mesh_bvh_build(T, tri.data(), leaf, h);
        std::vector<long long> visits((size_t)(4 * P), 0);
        for (int r = 0; r < 2; r++) {
            long long nts = 0, tts = 0, walked = 0;
            std::string why;
            for (int64_t i = 0; i < P && why.empty(); i++) {
                const double p[3] = {pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2]};
                double got = seeds[r];
                if (p[0] == p[0] && p[1] == p[1] && p[2] == p[2]) {
                    int nt = 0, tt = 0;
                    got = standoff_mesh_walk(h.nodes.data(), (int32_t)h.nodes.size(), h.tris.data(), p, seeds[r], nt, tt);
                    const double brute = standoff_mesh_brute(h.tris.data(), (int32_t)h.tris.size(), p, seeds[r]);
                    if (std::memcmp(&got, &brute, sizeof got) != 0)
                        why = "the walk and brute force differ on point " + std::to_string(i) + ": " + std::to_string(got) + " and " + std::to_string(brute);
                    visits[(size_t)((r * P + i) * 2)] = nt; visits[(size_t)((r * P + i) * 2 + 1)] = tt;
                    if (r == 1 && (visits[(size_t)(i * 2)] > nt || visits[(size_t)(i * 2 + 1)] > tt))
                        why = "the finite reach makes more tests than +Inf on point " + std::to_string(i);
                    nts += nt; tts += tt; walked++;
                }
                out[(size_t)(r * P + i)] = got;
            }
            if (why.empty() && leaf > 1 && std::memcmp(out.data() + r * P, first.data() + r * P, (size_t)P * sizeof(double)) != 0)
                why = "the values depend on the leaf size";
            if (why.empty())
                std::printf("leaf %d reach %s => ok node_tests %.1f tri_tests %.1f\n", leaf, r ? "inf" : argv[4], walked ? (double)nts / walked : 0.0,
                            walked ? (double)tts / walked : 0.0);
            else {
                std::printf("leaf %d reach %s => FAILED: %s\n", leaf, r ? "inf" : argv[4], why.c_str());
                bad = 1;
            }
        }
        if (leaf == 1) first = out;
    }
    FILE* f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(first.data(), sizeof(double), first.size(), f) != first.size()) { std::printf("cannot write %s\n", argv[3]); return 2; }
    std::fclose(f);
    return bad;
}
