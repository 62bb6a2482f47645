// The MLP classifier's step on the device (include/ocrl_hip_classifier.h).  The head is a chain of small Linear layers and runs on the
// actor-critic head's tile code (acnet_tile.h) as the Q head does (dqn.hip): a workgroup owns 16 batch rows, the chain's activations stay
// in LDS and the logits of the tile end in `lg`.
//   clf_ce            forward, soft-max cross-entropy, accuracy, dz and the backward per row tile in one kernel; z and the layer cotangents
//                     never leave LDS.  Partial dw go to the workgroup's slab, the three scalar sums to its row of scal_slab.  Evaluating,
//                     the tile stops after the loss
// Mean loss, accuracy and the count of valid rows come from the slabs' partial sums in slab order (dqn.hip's head_scalars); dw is folded
// by acnet_reduce.
// Order of every sum: acnet.hip's for the layers and the slabs; a row's exponentials are added in class order, a tile's scalar terms in
// row order, the tiles of a slab in tile order, the slabs in slab order.  No atomics.
#include "acnet_tile.h"
#include "classifier.h"

namespace {

// The loss of one tile after its forward: thread r < 16 owns row r (A <= 64: the scans are serial in a).  Adds the row's three terms
// (cross-entropy, hit, valid) to the slab's partial sums and, with `backward`, replaces the logits in lg by dL/dz (L = the sum of the
// rows' losses over B).  A row whose label is outside [0, A), or past the batch, adds nothing and gets a zero cotangent.
__device__ void ce_rows(const AcnetArgs& p, const ClfCeArgs& s, long long row0, int rows, bool first, float* lg, float (*rs)[3]) {
    const int r = threadIdx.x;
    if (r < TR) {
        float t[3] = {0.f, 0.f, 0.f};
        float* z = lg + r * LA;
        const int A = p.A;
        const long long y = r < rows ? s.labels[row0 + r] : -1;
        if (y >= 0 && y < A) {
            float m = z[0];
            int best = 0;
            for (int a = 1; a < A; ++a)
                if (z[a] > m) { m = z[a]; best = a; }   // strict: the lowest index of the maximum
            float sum = 0.f;
            for (int a = 0; a < A; ++a) sum += expf(z[a] - m);
            const float lse = m + logf(sum);
            t[0] = lse - z[y];
            t[1] = best == (int)y ? 1.f : 0.f;
            t[2] = 1.f;
            if (s.backward) {
                const float fB = (float)p.B;
                for (int a = 0; a < A; ++a) z[a] = (expf(z[a] - lse) - (a == (int)y ? 1.f : 0.f)) / fB;
            }
        } else if (s.backward) {
            for (int a = 0; a < A; ++a) z[a] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) rs[r][j] = t[j];
    }
    __syncthreads();
    tile_scalars<3>(rs, first, p.scal_slab);
}

__global__ __launch_bounds__(256) void clf_ce_kernel(AcnetArgs p, ClfCeArgs s) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    __shared__ float rs[TR][3];
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long row0 = (long long)tile * TR;
        const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
        const bool first = tile == (int)blockIdx.x;
        fwd_tile(p, row0, rows, buf, lg, nullptr);
        ce_rows(p, s, row0, rows, first, lg, rs);
        if (s.backward) {
            bwd_tile(p, row0, rows, first, buf, lg, nullptr);
            __syncthreads();
        }
    }
}

}  // namespace

int clf_ce_launch(const AcnetArgs& a, const ClfCeArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(clf_ce_kernel, dim3(a.S), dim3(256), 0, st, a, s);
    OCRL_CHECK_LAUNCH("clf_ce");
    return 0;
}
