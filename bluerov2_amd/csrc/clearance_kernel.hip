// clearance_kernel.hip -- the inter-vehicle clearance term of the fleet planning loop (include/bluerov2_nmpc.h, brov_clearance_*; DESIGN.md
// section 4.12b; the specification is tests/clearance_restatement.py).  Behind a solve, ahead of the fleet's select:
//   clearance_dist_kernel      per candidate b = v * C + c the squared distance of closest approach between its predicted path x[b][k][0..2]
//                              and the plans the OTHER vehicles committed to, plan[min(k + shift, N)][w], w != v
//   clearance_rescore_kernel   the records with cost += weight * (r2 - d2min) where d2min < r2, everything else copied
// and behind the select:
//   clearance_publish_kernel   the winner's path becomes its vehicle's plan (without a winner the old plan advances), the step's statistics
//
// clearance_dist_kernel: lane <-> candidate.  A block is four wavefronts over the SAME 64 consecutive candidates (whatever their vehicles);
// the peer range is cut into contiguous slices, one per wavefront of the block and per blockIdx.y.  A wavefront walks the stages k with its
// slice of the peers inside: the lane's own stage-k position sits in three registers, the plan point of (k, w) is the same for all 64 lanes
// -- a wave-uniform address, read through the scalar cache -- and the plan is stage-major so that the inner loop reads consecutive memory.
// The lane's own vehicle is masked out by index, never by distance.  The four wavefronts meet in LDS with a plain minimum; the grid-level
// slices are written side by side (part[slice][b]) and folded by clearance_rescore_kernel.  A minimum of non-NaN values does not depend on
// the order it is taken in (sums of squares are never -0.0), so the bytes do not depend on the launch geometry: no atomics, two calls
// return the same bytes.  Arithmetic in the stated order, products and sums rounded separately:
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cstddef>

#include "clearance_kernel.hpp"
#include "select_device.hpp"

namespace brov {

constexpr int kClearanceBlock = 256;
constexpr int kClearanceWaves = kClearanceBlock / 64;
constexpr int kNX = 12;   // doubles per stage of the iterate

// m := the lower of m and the squared distance of (px, py, pz) from the plan point (qx, qy, qz) of a vehicle that is a peer
__device__ __forceinline__ double clearance_fold(double m, double px, double py, double pz, double qx, double qy, double qz, bool peer) {
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    return peer && d2 < m ? d2 : m;   // a NaN distance compares false: skipped
}

__global__ __launch_bounds__(kClearanceBlock) void clearance_dist_kernel(const double* __restrict__ x, const double* __restrict__ plan, int B, int V,
                                                                         int C, int N, int shift, int per_wave, double* __restrict__ part) {
    __shared__ double red[kClearanceWaves][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x * 64 + lane;
    const int bc = b < B ? b : B - 1;   // the lanes past the batch walk the last candidate's path and store nothing: whole wavefronts reach the barrier
    const int v = bc / C;
    const int slice = blockIdx.y * kClearanceWaves + wave;
    const long long w0l = (long long)slice * per_wave;
    const int w0 = w0l < V ? (int)w0l : V;
    const int w1 = w0 + per_wave < V ? w0 + per_wave : V;
    const double* __restrict__ xs = x + (size_t)bc * (N + 1) * kNX;
    double m = __builtin_huge_val();
    double nx = xs[0], ny = xs[1], nz = xs[2];
    for (int k = 0; k <= N; k++) {
        const double px = nx, py = ny, pz = nz;
        const int kn = k < N ? k + 1 : N;   // the next stage's position is asked for ahead of this stage's walk over the peers
        nx = xs[(size_t)kn * kNX + 0]; ny = xs[(size_t)kn * kNX + 1]; nz = xs[(size_t)kn * kNX + 2];
        const int kp = k + shift < N ? k + shift : N;
        const double* __restrict__ p = plan + ((size_t)kp * V + w0) * 3;
        int w = w0;
        if (w + 4 <= w1) {
            // four peers at a time, the next four asked for ahead of the arithmetic on these: scalar loads return out of order, a wait for
            // one is a wait for all, and the wait at the head of an iteration is then for a load that had an iteration to arrive
            double q[12];
#pragma unroll
            for (int j = 0; j < 12; j++) q[j] = p[j];
            for (; w + 4 <= w1; w += 4) {
                double c[12];
#pragma unroll
                for (int j = 0; j < 12; j++) c[j] = q[j];
                p += 12;
                if (w + 8 <= w1) {
#pragma unroll
                    for (int j = 0; j < 12; j++) q[j] = p[j];
                }
#pragma unroll
                for (int i = 0; i < 4; i++) m = clearance_fold(m, px, py, pz, c[3 * i], c[3 * i + 1], c[3 * i + 2], w + i != v);
            }
        }
        for (; w < w1; w++, p += 3) m = clearance_fold(m, px, py, pz, p[0], p[1], p[2], w != v);
    }
    red[wave][lane] = m;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int i = 1; i < kClearanceWaves; i++) {
            const double t = red[i][lane];
            if (t < m) m = t;
        }
        if (b < B) part[(size_t)blockIdx.y * B + b] = m;
    }
}

// one thread per candidate.  rec and out may be the same array: a thread reads its record before it writes it
__global__ __launch_bounds__(256) void clearance_rescore_kernel(const double* __restrict__ part, int slices, int B, const brov_result* rec, double r2,
                                                                double weight, double* __restrict__ d2min, brov_result* out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double m = part[b];
    for (int s = 1; s < slices; s++) {
        const double t = part[(size_t)s * B + b];
        if (t < m) m = t;
    }
    d2min[b] = m;
    if (!out) return;
    unsigned long long word[kResultWords];
#pragma unroll
    for (int i = 0; i < kResultWords; i++) word[i] = result_word(rec + b, i);
    if (m < r2) {
        constexpr int kCostWord = (int)(offsetof(brov_result, cost) / 8);
        const double pen = weight * (r2 - m);
        const double old = __longlong_as_double((long long)word[kCostWord]);
        const double cost = old + pen;
        // a cost that is NaN already keeps its bytes (what the sum of a quiet NaN gives).  A NaN the sum GENERATES (-Inf + Inf) is written as
        // THE quiet NaN (sign 0, payload 0): IEEE leaves sign and payload of a generated NaN open (it is the negative one on x86), so no
        // processor's choice is part of the rule; the restatement writes the same word
        if (old == old) word[kCostWord] = cost != cost ? 0x7ff8000000000000ULL : (unsigned long long)__double_as_longlong(cost);
    }
#pragma unroll
    for (int i = 0; i < kResultWords; i++) result_word(out + b, i) = word[i];
}

// one thread per vehicle, the stages in ascending order: the advance plan[k] := plan[min(k + shift, N)] reads at or ahead of where it
// writes, and nobody else touches the vehicle's column.  Consecutive threads touch consecutive 24-byte points of a stage.
__global__ __launch_bounds__(128) void clearance_publish_kernel(const double* __restrict__ x, const int32_t* __restrict__ winner,
                                                                const double* __restrict__ d2min, int V, int C, int N, int shift, double r2,
                                                                double* plan, double* __restrict__ last_d2, double* __restrict__ min_d2,
                                                                int32_t* __restrict__ below) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int win = winner[v];
    if (win >= 0) {
        const size_t b = (size_t)v * C + win;
        const double* __restrict__ xs = x + b * (N + 1) * kNX;
        for (int k = 0; k <= N; k++) {
            double* q = plan + ((size_t)k * V + v) * 3;
            q[0] = xs[(size_t)k * kNX + 0]; q[1] = xs[(size_t)k * kNX + 1]; q[2] = xs[(size_t)k * kNX + 2];
        }
        const double d = d2min[b];
        last_d2[v] = d;
        if (d < min_d2[v]) min_d2[v] = d;
        if (d < r2) below[v] += 1;
    } else {
        if (shift > 0) {
            for (int k = 0; k <= N; k++) {
                const int kp = k + shift < N ? k + shift : N;
                const double* s = plan + ((size_t)kp * V + v) * 3;
                double* q = plan + ((size_t)k * V + v) * 3;
                const double s0 = s[0], s1 = s[1], s2 = s[2];
                q[0] = s0; q[1] = s1; q[2] = s2;
            }
        }
        last_d2[v] = -1.0;
    }
}

int clearance_slices(int B, int V) {
    const int groups = (B + 63) / 64;
    const int want = (2048 + groups * kClearanceWaves - 1) / (groups * kClearanceWaves);   // 2048 wavefronts: two per SIMD of 256 compute units
    const int have = (V + kClearanceWaves - 1) / kClearanceWaves;                           // at least one peer per wavefront
    int s = want < have ? want : have;
    if (s > kClearanceMaxSlices) s = kClearanceMaxSlices;
    return s < 1 ? 1 : s;
}

void launch_clearance_dist(const double* x, const double* plan, int B, int V, int C, int N, int shift, int slices, double* part, hipStream_t st) {
    const int waves = slices * kClearanceWaves;
    const int per_wave = (V + waves - 1) / waves;
    hipLaunchKernelGGL(clearance_dist_kernel, dim3((unsigned)((B + 63) / 64), (unsigned)slices), dim3(kClearanceBlock), 0, st, x, plan, B, V, C, N,
                       shift, per_wave, part);
}
void launch_clearance_rescore(const double* part, int slices, int B, const brov_result* rec, double r2, double weight, double* d2min,
                              brov_result* out, hipStream_t st) {
    hipLaunchKernelGGL(clearance_rescore_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, part, slices, B, rec, r2, weight, d2min, out);
}
void launch_clearance_publish(const double* x, const int32_t* winner, const double* d2min, int V, int C, int N, int shift, double r2, double* plan,
                              double* last_d2, double* min_d2, int32_t* below, hipStream_t st) {
    hipLaunchKernelGGL(clearance_publish_kernel, dim3((unsigned)((V + 127) / 128)), dim3(128), 0, st, x, winner, d2min, V, C, N, shift, r2, plan,
                       last_d2, min_d2, below);
}

}  // namespace brov
