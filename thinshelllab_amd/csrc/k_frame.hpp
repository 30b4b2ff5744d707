// Rigid frames for soft handles (tsl_set_handle_frames): handle i may belong to frame f_i with a local point r_i; frame j has a
// pose (c_j, R_j) and the target of a framed handle is t_i = c_j + R_j r_i.  The frames rewrite rows of the target buffer the handle kernels
// (k_handle.hpp) read, and reduce per-handle rows to six numbers per frame; nothing here runs inside a step, an energy, an assembly or a reverse
// step.  No atomics: every target row has one writer, every frame one workgroup that adds in a fixed order -- the same bits run to run.
#pragma once
#include "k_handle.hpp"
#include "tsl_device.hpp"

struct FrameArgs {
  int n_frame;
  const int* of;         // n_handle      frame of handle i, -1: a free handle (world target)
  const double* local;   // n_handle x 3  r_i (not read for free handles)
  const double* c;       // n_frame x 3   position
  const double* R;       // n_frame x 9   rotation, row-major
  const int* ptr;        // n_frame + 1   CSR of the handles of every frame,
  const int* idx;        //               handle numbers ascending within a frame
};

// t_i = c + R r_i for the framed handles; rows of free handles keep their value.  One lane per handle, plain loads and stores.  Contraction is off:
// the row is the three products added left to right, then c, whatever the compiler -- the NumPy statement of the same order gives the same bits.
__global__ void k_frame_targets(int n_handle, FrameArgs A, double* __restrict__ t) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_handle) return;
  const int f = A.of[i];
  if (f < 0) return;
  const d3 r = ld3(A.local, i), c = ld3(A.c, f);
  const double* __restrict__ R = A.R + 9 * (size_t)f;
  st3(t, i, d3(c.x + ((R[0] * r.x + R[1] * r.y) + R[2] * r.z), c.y + ((R[3] * r.x + R[4] * r.y) + R[5] * r.z), c.z + ((R[6] * r.x + R[7] * r.y) + R[8] * r.z)));
}

// Six sums per frame, one 256-lane workgroup per frame: out[6 j ..] = (sum_i f_i, sum_i a_i x f_i) over the frame's handles.
//   FRAME_WRENCH: f_i = k w_i (t_i - p_i), the row of k_handle_force (frozen dofs not masked), a_i = t_i - c_j: force and moment about c_j that
//                 the frame's handles apply to the cloth, = dE_h / d(c_j, theta_j);  vec = positions.
//   FRAME_GRAD:   f_i = the row of k_handle_backprop (k w_i sum_a b_a p_{v_a} on free dofs, 0 on frozen ones), a_i = R_j r_i: one reverse step's
//                 contribution to d(loss) / d(c_j, theta_j), theta a world-frame rotation vector applied on the left;  vec = the adjoint solution p.
// Lane l takes the entries l, l + 256, ... of the frame's list in ascending order; the lanes are joined by wg_join (the join of k_handle_energy,
// six sums at once).  A frame without handles stores six zeros.  NC: the corners per handle of the list (k_handle.hpp).
enum { FRAME_WRENCH = 0, FRAME_GRAD = 1 };
template <int MODE, int NC>
__global__ void __launch_bounds__(256) k_frame_reduce(HandleArgs H, FrameArgs A, const double* __restrict__ vec, const int* __restrict__ frozen,
                                                      double* __restrict__ out) {
  const int j = blockIdx.x;
  const int e1 = A.ptr[j + 1];
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double* __restrict__ R = A.R + 9 * (size_t)j;
  const d3 c = MODE == FRAME_WRENCH ? ld3(A.c, j) : d3(0.0, 0.0, 0.0);   // (the wrench's arms start at c; the gradient's are R r)
  for (int e = A.ptr[j] + (int)threadIdx.x; e < e1; e += 256) {
    const int i = A.idx[e];
    d3 f, a;
    if (MODE == FRAME_WRENCH) {
      const d3 t = ld3(H.t, i);
      f = (t - handle_point<NC>(H, vec, i)) * (H.k * H.w[i]);
      a = t - c;
    } else {
      const d3 r = ld3(A.local, i);
      f = handle_backprop_row<NC>(H, vec, frozen, i);
      a = d3(R[0] * r.x + R[1] * r.y + R[2] * r.z, R[3] * r.x + R[4] * r.y + R[5] * r.z, R[6] * r.x + R[7] * r.y + R[8] * r.z);
    }
    const d3 m = cross(a, f);
    s[0] += f.x; s[1] += f.y; s[2] += f.z;
    s[3] += m.x; s[4] += m.y; s[5] += m.z;
  }
  wg_join<6>(s, out + 6 * (size_t)j);
}
