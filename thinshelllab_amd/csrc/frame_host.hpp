// Host side of rigid frames for soft handles (tsl_set_handle_frames / tsl_set_frame_poses): the checks of the lists, the list of
// handles per frame and the pose (c, q) -> (c, R).  Plain C++ with no device code, so that it can also be compiled into a stand-alone program
// (a CPU build under a sanitizer) without the rest of the library.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

// 0: the lists are valid.  -1: err names the offender -- frames asked for while there are no handles, a frame index outside [-1, n_frame), a
// non-finite local point of a framed handle (the point of a free handle, frame -1, is never read).  n_frame = 0 (remove all frames) reads no list.
inline int frame_validate(int n_handle, const int32_t* frame_of, const double* local, int32_t n_frame, std::string& err) {
  char buf[256];
  if (n_frame < 0) { snprintf(buf, sizeof(buf), "n_frame = %d is negative", n_frame); err = buf; return -1; }
  if (n_frame == 0) return 0;
  if (n_handle <= 0) { snprintf(buf, sizeof(buf), "%d frames asked for, but there are no handles (tsl_set_handles comes first)", n_frame); err = buf; return -1; }
  if (!frame_of || !local) { err = "null frame list or null local points"; return -1; }
  for (int i = 0; i < n_handle; i++) {
    const int f = frame_of[i];
    if (f < -1 || f >= n_frame) { snprintf(buf, sizeof(buf), "frame index %d of handle %d outside [-1, %d)", f, i, n_frame); err = buf; return -1; }
    if (f < 0) continue;
    const double* r = local + 3 * (size_t)i;
    if (!(std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]))) {
      snprintf(buf, sizeof(buf), "local point (%g, %g, %g) of handle %d (frame %d) is not finite", r[0], r[1], r[2], i, f); err = buf; return -1;
    }
  }
  return 0;
}

// The handles of every frame as a CSR: frame j owns idx[ptr[j] .. ptr[j + 1]), handle numbers ascending (a counting sort over the handles in order),
// free handles in no list.  The lists are valid (frame_validate).
inline void frame_csr(int n_handle, const int32_t* frame_of, int32_t n_frame, std::vector<int>& ptr, std::vector<int>& idx) {
  ptr.assign((size_t)n_frame + 1, 0);
  for (int i = 0; i < n_handle; i++)
    if (frame_of[i] >= 0) ptr[(size_t)frame_of[i] + 1]++;
  for (int j = 0; j < n_frame; j++) ptr[(size_t)j + 1] += ptr[j];
  idx.assign((size_t)ptr[n_frame], 0);
  std::vector<int> fill(ptr.begin(), ptr.end() - 1);
  for (int i = 0; i < n_handle; i++)
    if (frame_of[i] >= 0) idx[(size_t)fill[frame_of[i]]++] = i;
}

// Poses: c (n_frame x 3) copied, every quaternion q = (s, x, y, z) normalised and turned into the row-major R of engine/gripper_single.quat_to_rotmat
// (n_frame x 9).  -1 and err names the frame for a zero or non-finite quaternion or a non-finite position.
inline int frame_pose_matrices(const double* pos, const double* quat, int32_t n_frame, std::vector<double>& c, std::vector<double>& R, std::string& err) {
#pragma clang fp contract(off)
  char buf[256];
  if (n_frame > 0 && (!pos || !quat)) { err = "null positions or null quaternions"; return -1; }
  c.assign(3 * (size_t)n_frame, 0.0);
  R.assign(9 * (size_t)n_frame, 0.0);
  for (int j = 0; j < n_frame; j++) {
    const double* p = pos + 3 * (size_t)j;
    const double* q = quat + 4 * (size_t)j;
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) {
      snprintf(buf, sizeof(buf), "position (%g, %g, %g) of frame %d is not finite", p[0], p[1], p[2], j); err = buf; return -1;
    }
    const double n = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    if (!(n > 0.0) || !std::isfinite(n)) {
      snprintf(buf, sizeof(buf), "quaternion (%g, %g, %g, %g) of frame %d is zero or not finite", q[0], q[1], q[2], q[3], j); err = buf; return -1;
    }
    const double s = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    for (int a = 0; a < 3; a++) c[3 * (size_t)j + a] = p[a];
    double* M = R.data() + 9 * (size_t)j;
    M[0] = s * s + x * x - y * y - z * z; M[1] = 2 * (x * y - s * z);           M[2] = 2 * (x * z + s * y);
    M[3] = 2 * (x * y + s * z);           M[4] = s * s - x * x + y * y - z * z; M[5] = 2 * (y * z - s * x);
    M[6] = 2 * (x * z - s * y);           M[7] = 2 * (y * z + s * x);           M[8] = s * s - x * x - y * y + z * z;
  }
  return 0;
}
