// render_camera.h -- the camera matrices of the renderer (include/rgbdfe.h, "rendering"): plain host C++ in
// double, no HIP.  api_render.hip exports these as rgbdfe_render_perspective / _viewer_view / _sensor_camera / _unproject;
// tests/test_oracle_render.py compiles this header alone and holds it against tests/render_oracle.py byte for byte.
// Matrices are 16 doubles, column-major (m[4 * column + row]).  Sums of products run left to right.
#pragma once
#include <cmath>

namespace rgbdfe {

constexpr double kRenderPi = 3.14159265358979323846;

// out = a * b
inline void render_mat_mul(const double* a, const double* b, double* out) {
  double r[16];
  for (int c = 0; c < 4; ++c)
    for (int i = 0; i < 4; ++i)
      r[4 * c + i] = ((a[i] * b[4 * c] + a[4 + i] * b[4 * c + 1]) + a[8 + i] * b[4 * c + 2]) + a[12 + i] * b[4 * c + 3];
  for (int i = 0; i < 16; ++i) out[i] = r[i];
}

inline void render_identity(double* m) {
  for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

// gluPerspective(fovy, aspect, z_near, z_far): fovy in degrees
inline void render_perspective(double fovy, double aspect, double z_near, double z_far, double* m) {
  const double rad = fovy / 2.0 * kRenderPi / 180.0;
  const double cot = std::cos(rad) / std::sin(rad);
  for (int i = 0; i < 16; ++i) m[i] = 0.0;
  m[0] = cot / aspect;
  m[5] = cot;
  m[10] = -(z_far + z_near) / (z_far - z_near);
  m[11] = -1.0;
  m[14] = -(2.0 * z_far * z_near) / (z_far - z_near);
}

// glRotatef(angle, axis) for a coordinate axis (0 x, 1 y, 2 z): the angle is taken as the float GL receives
inline void render_axis_rotation(double angle_deg, int axis, double* m) {
  const double a = (double)(float)angle_deg * kRenderPi / 180.0;
  const double c = std::cos(a), s = std::sin(a);
  render_identity(m);
  const int i = (axis + 1) % 3, j = (axis + 2) % 3;
  m[4 * i + i] = c;
  m[4 * j + j] = c;
  m[4 * i + j] = s;   // row j, column i
  m[4 * j + i] = -s;  // row i, column j
}

// GLViewer::drawClouds' modelview (glviewer.cpp:356-377): glTranslatef, the three stepped glRotatef, glMultMatrix(viewpoint)
inline void render_viewer_view(double x_tra, double y_tra, double z_tra, double x_rot, double y_rot, double z_rot,
                               double rotation_stepping, const double* viewpoint, double* m) {
  double t[16], r[16];
  render_identity(t);
  t[12] = (double)(float)x_tra;
  t[13] = (double)(float)y_tra;
  t[14] = (double)(float)z_tra;
  const double rot[3] = {x_rot, y_rot, z_rot};
  for (int axis = 0; axis < 3; ++axis) {
    const int steps = (int)((rot[axis] / 16.0) / rotation_stepping);  // `int x_steps = (xRot / 16.0)/rotation_stepping_`
    render_axis_rotation(steps * rotation_stepping, axis, r);
    render_mat_mul(t, r, t);
  }
  if (viewpoint) {
    render_mat_mul(t, viewpoint, t);
  }
  for (int i = 0; i < 16; ++i) m[i] = t[i];
}

// The view and projection under which the point (x, y, z) of the sensor frame at the rigid `pose` (z forward, y down) lands
// at x_w = fx x / z + cx + 1/2 and at image row fy y / z + cy + 1/2 from the top (y_w = H - that).
inline void render_sensor_camera(double fx, double fy, double cx, double cy, int W, int H, double z_near, double z_far,
                                 const double* pose, double* view, double* projection) {
  // eye = diag(1, -1, -1) * (R^T (p - t))
  double inv[16];
  render_identity(inv);
  if (pose) {
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) inv[4 * c + r] = pose[4 * r + c];
      inv[12 + r] = -((pose[4 * r] * pose[12] + pose[4 * r + 1] * pose[13]) + pose[4 * r + 2] * pose[14]);
    }
  }
  for (int c = 0; c < 4; ++c) {
    view[4 * c] = inv[4 * c];
    view[4 * c + 1] = -inv[4 * c + 1];
    view[4 * c + 2] = -inv[4 * c + 2];
    view[4 * c + 3] = inv[4 * c + 3];
  }
  for (int i = 0; i < 16; ++i) projection[i] = 0.0;
  projection[0] = 2.0 * fx / W;
  projection[5] = 2.0 * fy / H;
  projection[8] = 1.0 - 2.0 * (cx + 0.5) / W;
  projection[9] = 2.0 * (cy + 0.5) / H - 1.0;
  projection[10] = -(z_far + z_near) / (z_far - z_near);
  projection[11] = -1.0;
  projection[14] = -(2.0 * z_far * z_near) / (z_far - z_near);
}

// gluUnProject over the viewport (0, 0, W, H): the inverse of projection * view by Gauss-Jordan elimination with partial
// pivoting.  Returns 0 when the product is singular or the result's w is 0 (out untouched), else 1.
inline int render_unproject(double x, double y, double depth, const double* view, const double* projection, int W, int H,
                            double* out) {
  double a[16], m[4][8];
  render_mat_mul(projection, view, a);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      m[r][c] = a[4 * c + r];
      m[r][4 + c] = (r == c) ? 1.0 : 0.0;
    }
  for (int k = 0; k < 4; ++k) {
    int p = k;
    for (int r = k + 1; r < 4; ++r)
      if (std::fabs(m[r][k]) > std::fabs(m[p][k])) p = r;
    if (m[p][k] == 0.0) return 0;
    if (p != k)
      for (int c = 0; c < 8; ++c) {
        const double t = m[k][c];
        m[k][c] = m[p][c];
        m[p][c] = t;
      }
    const double d = m[k][k];
    for (int c = 0; c < 8; ++c) m[k][c] = m[k][c] / d;
    for (int r = 0; r < 4; ++r) {
      if (r == k) continue;
      const double f = m[r][k];
      for (int c = 0; c < 8; ++c) m[r][c] = m[r][c] - f * m[k][c];
    }
  }
  const double in[4] = {x / W * 2.0 - 1.0, y / H * 2.0 - 1.0, depth * 2.0 - 1.0, 1.0};
  double o[4];
  for (int r = 0; r < 4; ++r) o[r] = ((m[r][4] * in[0] + m[r][5] * in[1]) + m[r][6] * in[2]) + m[r][7] * in[3];
  if (o[3] == 0.0) return 0;
  out[0] = o[0] / o[3];
  out[1] = o[1] / o[3];
  out[2] = o[2] / o[3];
  return 1;
}

}  // namespace rgbdfe
