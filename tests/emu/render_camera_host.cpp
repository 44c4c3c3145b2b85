// tests/emu/render_camera_host.cpp -- TEST INFRASTRUCTURE ONLY: csrc/render_camera.h (plain host C++, no HIP) behind a C
// interface, so that tests/test_oracle_render.py can hold the library's camera helpers against tests/render_oracle.py on a
// machine without a device.  librgbdfe.so exports the same functions as rgbdfe_render_*.
#include "render_camera.h"

extern "C" {
void host_perspective(double fovy, double aspect, double z_near, double z_far, double* out) {
  rgbdfe::render_perspective(fovy, aspect, z_near, z_far, out);
}
void host_viewer_view(double x_tra, double y_tra, double z_tra, double x_rot, double y_rot, double z_rot, double stepping,
                      const double* viewpoint, double* out) {
  rgbdfe::render_viewer_view(x_tra, y_tra, z_tra, x_rot, y_rot, z_rot, stepping, viewpoint, out);
}
void host_sensor_camera(double fx, double fy, double cx, double cy, int W, int H, double z_near, double z_far, const double* pose,
                        double* view, double* projection) {
  rgbdfe::render_sensor_camera(fx, fy, cx, cy, W, H, z_near, z_far, pose, view, projection);
}
int host_unproject(double x, double y, double depth, const double* view, const double* projection, int W, int H, double* out) {
  return rgbdfe::render_unproject(x, y, depth, view, projection, W, H, out);
}
}
