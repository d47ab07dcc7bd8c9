// mesh_bvh_main.cpp -- the builder of the range stage's mesh hierarchy (bluerov2_amd/csrc/mesh_bvh.hpp) on the host alone, for
// tests/test_mesh_bvh_cpu.py, which compiles this file with -fsanitize=address,undefined and runs it directly.  Arguments: files of raw
// float64 triangles [T][3][3].  For every file and every leaf size 1 ... 8 it builds the structure and checks
//   - every triangle is in exactly one leaf, a leaf holds 1 ... leaf triangles, and the stored triangles are those of the file in leaf order
//   - every node box contains the vertices of its subtree and the pad
//   - skip links strictly increase, a leaf's is the next index, the root's is the node count, none points past it
//   - depth <= ceil(log2 T) + 1
//   - a forward walk with the kernels' visit test gives, on rays from inside the mesh's bounds, exactly the smallest hit t of testing every
//     triangle (the structure's only contract; the arithmetic here is plain host doubles, compiled without contraction)
// and prints "<file> leaf <l> => ok nodes <n> leaves <n> depth <d> node_tests <mean> tri_tests <mean>" or the first failure.  Exit code 1 on a failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mesh_bvh.hpp"

using namespace brov;

static void cross(const double* a, const double* b, double* r) {
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}
static double dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static bool tri_hit(const MeshTri& T, const double* o, const double* D, double near, double far, double* t_out) {
    double p[3], s[3], q[3];
    cross(D, T.e2, p);
    const double det = dot(T.e1, p), inv = 1.0 / det;
    for (int c = 0; c < 3; c++) s[c] = o[c] - T.v0[c];
    const double u = dot(s, p) * inv;
    cross(s, T.e1, q);
    const double v = dot(D, q) * inv, t = dot(T.e2, q) * inv;
    *t_out = t;
    return det != 0.0 && u >= 0.0 && v >= 0.0 && u + v <= 1.0 && t >= near && t <= far;
}

static std::string check(const std::vector<double>& tri, int leaf, std::string& report) {
    const int64_t n = (int64_t)tri.size() / 9;
    MeshBvh h;
    mesh_bvh_build(n, tri.data(), leaf, h);
    const int N = (int)h.nodes.size();
    if (N < 1 || (int64_t)h.tris.size() != n || (int64_t)h.order.size() != n) return "sizes";
    // leaves tile [0, n) in index order; the order is a permutation
    std::vector<int> seen((size_t)n, 0);
    for (int32_t k : h.order) {
        if (k < 0 || k >= n) return "order out of range";
        seen[(size_t)k]++;
    }
    for (int v : seen)
        if (v != 1) return "a triangle is not in exactly one leaf";
    int next = 0, leaves = 0;
    for (int i = 0; i < N; i++) {
        const MeshNode& nd = h.nodes[i];
        if (nd.skip <= i || nd.skip > N) return "a skip link does not increase or points past the end";
        if (nd.count < 0 || nd.count > leaf) return "a leaf holds more than leaf triangles";
        if (nd.count > 0) {
            if (nd.first != next) return "the leaves do not tile the triangles in order";
            if (nd.skip != i + 1) return "a leaf's skip link is not the next index";
            next += nd.count;
            leaves++;
        } else if (nd.skip < i + 3) return "an interior node without two children";
    }
    if (next != n || leaves != h.leaves) return "the leaves do not cover the triangles";
    if (h.nodes[0].skip != N) return "the root's skip link is not the node count";
    for (int64_t k = 0; k < n; k++) {
        const MeshTri want = mesh_stored_triangle(tri.data() + (size_t)h.order[(size_t)k] * 9);
        for (int c = 0; c < 3; c++)
            if (want.v0[c] != h.tris[(size_t)k].v0[c] || want.e1[c] != h.tris[(size_t)k].e1[c] || want.e2[c] != h.tris[(size_t)k].e2[c]) return "a stored triangle differs";
    }
    // boxes: the subtree of node i is the nodes [i, skip)
    double ext = 0.0;
    {
        double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
        for (size_t j = 0; j < tri.size(); j++) { lo[j % 3] = std::fmin(lo[j % 3], tri[j]); hi[j % 3] = std::fmax(hi[j % 3], tri[j]); }
        for (int c = 0; c < 3; c++) ext = std::fmax(ext, hi[c] - lo[c]);
    }
    if (h.pad != std::ldexp(ext, -30)) return "the pad is not 2^-30 x the largest extent";
    for (int i = 0; i < N; i++) {
        const MeshNode& nd = h.nodes[i];
        for (int j = i; j < nd.skip; j++) {
            const MeshNode& lf = h.nodes[j];
            for (int k = lf.first; k < lf.first + lf.count; k++) {
                const double* t = tri.data() + (size_t)h.order[(size_t)k] * 9;
                for (int v = 0; v < 9; v++)
                    if (!(nd.lo[v % 3] <= t[v] - h.pad && nd.hi[v % 3] >= t[v] + h.pad)) return "a node box does not contain its subtree and the pad";
            }
        }
    }
    int bound = 1;
    while ((1LL << (bound - 1)) < n) bound++;   // ceil(log2 n) + 1
    if (h.depth > bound) return "depth above ceil(log2 T) + 1";
    // the walk against brute force: rays from the middle of the bounds, a fixed pseudo-random set of directions
    const double near = 1e-3, far = 1e6, inf = HUGE_VAL;
    double o[3];
    for (int c = 0; c < 3; c++) o[c] = 0.5 * (h.nodes[0].lo[c] + h.nodes[0].hi[c]) + 0.013 * (c + 1) * ext;
    unsigned long long z = 0x9E3779B97F4A7C15ULL;
    long long nt = 0, tt = 0;
    const int rays = 200;
    for (int r = 0; r < rays; r++) {
        double D[3], inv[3];
        for (int c = 0; c < 3; c++) {
            z ^= z << 13; z ^= z >> 7; z ^= z << 17;
            D[c] = (double)(long long)(z >> 11) * 0x1.0p-52 - 1.0;
        }
        if (r % 10 == 0) D[r / 10 % 3] = 0.0;   // axis-parallel slabs as well
        for (int c = 0; c < 3; c++) inv[c] = 1.0 / D[c];
        double brute = inf, best = inf, t;
        for (const MeshTri& T : h.tris)
            if (tri_hit(T, o, D, near, far, &t) && t < brute) brute = t;
        int i = 0;
        while (i < N) {
            const MeshNode& nd = h.nodes[i];
            double tn = -inf, tf = inf;
            for (int c = 0; c < 3; c++) {
                const double t1 = (nd.lo[c] - o[c]) * inv[c], t2 = (nd.hi[c] - o[c]) * inv[c];
                tn = std::fmax(tn, std::fmin(t1, t2));
                tf = std::fmin(tf, std::fmax(t1, t2));
            }
            nt++;
            if (!(tn <= tf) || tf < near || tn > std::fmin(best, far)) { i = nd.skip; continue; }
            for (int k = nd.first; k < nd.first + nd.count; k++) {
                tt++;
                if (tri_hit(h.tris[(size_t)k], o, D, near, far, &t) && t < best) best = t;
            }
            i = nd.count > 0 ? nd.skip : i + 1;
        }
        if (!(best == brute)) return "the walk and brute force differ on ray " + std::to_string(r);
    }
    char buf[160];
    std::snprintf(buf, sizeof buf, "ok nodes %d leaves %d depth %d node_tests %.1f tri_tests %.1f", N, h.leaves, h.depth, (double)nt / rays, (double)tt / rays);
    report = buf;
    return "";
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; a++) {
        std::vector<double> tri;
        FILE* f = std::fopen(argv[a], "rb");
        if (!f) { std::printf("%s => cannot open\n", argv[a]); return 2; }
        double buf[9];
        while (std::fread(buf, sizeof(double), 9, f) == 9) tri.insert(tri.end(), buf, buf + 9);
        std::fclose(f);
        for (int leaf = 1; leaf <= 8; leaf++) {
            std::string report;
            const std::string why = check(tri, leaf, report);
            std::printf("%s leaf %d => %s\n", argv[a], leaf, why.empty() ? report.c_str() : ("FAILED: " + why).c_str());
            if (!why.empty()) bad = 1;
        }
    }
    return bad;
}
