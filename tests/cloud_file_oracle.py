"""Oracle of the map files (include/rgbdfe.h, "map files"; csrc/cloud_file_format.h): a numpy writer and an independent
reader for the binary PCD and the binary PLY layout, and the text of saveIndividualCloudsToFile's viewpoint and .txt.

The formats are restated from PCL 1.7's writers, not pinned on PCL's compiled code: the two header literals below are the
contract.  The writer builds a file from the literals and from array bytes; the reader does not share code with it: it takes
the header's length from the text (the line `DATA binary` / `end_header`), the counts from the lines it splits, and reads a
PLY's vertices through a structured dtype.

Clouds are float32 arrays whose last axis is (x, y, z, rgb bits); the rgb column only ever moves as a 32-bit word."""
import numpy as np

PCD_HEADER = ("# .PCD v0.7 - Point Cloud Data file format\n"
              "VERSION 0.7\n"
              "FIELDS x y z rgb\n"
              "SIZE 4 4 4 4\n"
              "TYPE F F F F\n"
              "COUNT 1 1 1 1\n"
              "WIDTH %d\n"
              "HEIGHT %d\n"
              "VIEWPOINT %s %s %s %s %s %s %s\n"
              "POINTS %d\n"
              "DATA binary\n")

PLY_HEADER = ("ply\n"
              "format binary_little_endian 1.0\n"
              "comment PCL generated\n"
              "element vertex %d\n"
              "property float x\n"
              "property float y\n"
              "property float z\n"
              "property uchar red\n"
              "property uchar green\n"
              "property uchar blue\n"
              "element camera 1\n"
              "property float view_px\n"
              "property float view_py\n"
              "property float view_pz\n"
              "property float x_axisx\n"
              "property float x_axisy\n"
              "property float x_axisz\n"
              "property float y_axisx\n"
              "property float y_axisy\n"
              "property float y_axisz\n"
              "property float z_axisx\n"
              "property float z_axisy\n"
              "property float z_axisz\n"
              "property float focal\n"
              "property float scalex\n"
              "property float scaley\n"
              "property float centerx\n"
              "property float centery\n"
              "property int viewportx\n"
              "property int viewporty\n"
              "property float k1\n"
              "property float k2\n"
              "end_header\n")

AGGREGATE_VIEWPOINT = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)   # ox oy oz qw qx qy qz
PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
PLY_CAMERA = np.dtype([("f", "<f4", 17), ("viewportx", "<i4"), ("viewporty", "<i4"), ("k", "<f4", 2)])
assert PLY_VERTEX.itemsize == 15 and PLY_CAMERA.itemsize == 84


def fmt_g(v):
    """A float as a C++ stream prints it by default: printf("%g") of the value."""
    return "%g" % float(np.float32(v))


def _rows(cloud):
    pts = np.ascontiguousarray(cloud, np.float32)
    assert pts.shape[-1] == 4
    height, width = (1, pts.shape[0]) if pts.ndim == 2 else pts.shape[:2]
    return pts.reshape(-1, 4), int(width), int(height)


def pcd_header(width, height, viewpoint=AGGREGATE_VIEWPOINT):
    return (PCD_HEADER % ((width, height) + tuple(fmt_g(v) for v in viewpoint) + (width * height,))).encode("ascii")


def pcd_bytes(cloud, viewpoint=AGGREGATE_VIEWPOINT):
    """[n, 4] -> WIDTH n, HEIGHT 1; [rows, cols, 4] -> WIDTH cols, HEIGHT rows."""
    pts, width, height = _rows(cloud)
    return pcd_header(width, height, viewpoint) + pts.tobytes()


def pack_ply(cloud):
    """n rows of 16 bytes -> 15 n bytes: x, y, z as they are, then bits 23-16, 15-8 and 7-0 of the rgb word."""
    pts, _, _ = _rows(cloud)
    v = np.zeros(len(pts), PLY_VERTEX)
    words = pts.view(np.uint32)
    for k, name in enumerate(("x", "y", "z")):
        v[name].view(np.uint32)[...] = words[:, k]
    v["red"] = (words[:, 3] >> 16) & 0xFF
    v["green"] = (words[:, 3] >> 8) & 0xFF
    v["blue"] = words[:, 3] & 0xFF
    return v.tobytes()


def pack_ply_scalar(cloud):
    """The same through a loop over rows and bytes."""
    pts, _, _ = _rows(cloud)
    raw = pts.tobytes()
    out = bytearray()
    for i in range(len(pts)):
        row = raw[16 * i:16 * i + 16]
        rgb = int.from_bytes(row[12:16], "little")
        out += row[:12] + bytes([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255])
    return bytes(out)


def ply_camera(width, height):
    cam = np.zeros(1, PLY_CAMERA)
    cam["f"][0, 3] = cam["f"][0, 7] = cam["f"][0, 11] = 1.0   # the identity row by row behind the origin
    cam["viewportx"], cam["viewporty"] = width, height
    return cam.tobytes()


def ply_bytes(cloud):
    pts, width, height = _rows(cloud)
    return (PLY_HEADER % len(pts)).encode("ascii") + pack_ply(pts) + ply_camera(width, height)


def file_bytes(cloud, fmt, viewpoint=AGGREGATE_VIEWPOINT):
    return pcd_bytes(cloud, viewpoint) if fmt == "pcd" else ply_bytes(cloud)


def read(data):
    """The independent reader: (points [height, width, 4] float32, info dict).  Raises ValueError on anything that is not
    one of the two layouts."""
    if data[:4] == b"ply\n":
        end = data.find(b"end_header\n")
        if end < 0:
            raise ValueError("no end_header")
        end += len(b"end_header\n")
        lines = data[:end].decode("ascii").split("\n")
        if lines[1] != "format binary_little_endian 1.0":
            raise ValueError("format")
        n = int(lines[3].split()[2])
        props = [ln for ln in lines if ln.startswith("property")]
        if lines[3].split()[:2] != ["element", "vertex"] or len(props) != 27 or \
                [p.split()[1:] for p in props[:6]] != [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"],
                                                       ["uchar", "green"], ["uchar", "blue"]]:
            raise ValueError("properties")
        if len(data) != end + 15 * n + 84:
            raise ValueError("length")
        v = np.frombuffer(data, PLY_VERTEX, n, end)
        cam = np.frombuffer(data, PLY_CAMERA, 1, end + 15 * n)
        width, height = int(cam["viewportx"][0]), int(cam["viewporty"][0])
        if width * height != n:
            raise ValueError("viewport")
        words = np.zeros((n, 4), np.uint32)
        for k, name in enumerate(("x", "y", "z")):
            words[:, k] = v[name].view(np.uint32)
        words[:, 3] = (v["red"].astype(np.uint32) << 16) | (v["green"].astype(np.uint32) << 8) | v["blue"]
        info = dict(format="ply", width=width, height=height, points=n, header_bytes=end, viewpoint=np.array(AGGREGATE_VIEWPOINT, np.float32),
                    camera=cam)
        return words.view(np.float32).reshape(height, width, 4), info
    end = data.find(b"DATA binary\n")
    if end < 0:
        raise ValueError("no DATA binary")
    end += len(b"DATA binary\n")
    fields = {}
    for ln in data[:end].decode("ascii").split("\n")[1:-1]:
        key, _, rest = ln.partition(" ")
        fields[key] = rest
    if (fields["VERSION"], fields["FIELDS"], fields["SIZE"], fields["TYPE"], fields["COUNT"]) != \
            ("0.7", "x y z rgb", "4 4 4 4", "F F F F", "1 1 1 1"):
        raise ValueError("fields")
    width, height, n = int(fields["WIDTH"]), int(fields["HEIGHT"]), int(fields["POINTS"])
    if width * height != n or len(data) != end + 16 * n:
        raise ValueError("length")
    pts = np.frombuffer(data, "<f4", 4 * n, end).reshape(height, width, 4)
    info = dict(format="pcd", width=width, height=height, points=n, header_bytes=end,
                viewpoint=np.array([float(t) for t in fields["VIEWPOINT"].split()], np.float32), viewpoint_text=fields["VIEWPOINT"])
    return pts, info


# ---- saveIndividualCloudsToFile (graph_mgr_io.cpp:330-433): the viewpoint and the .txt of one node -------------------------
def quat_from_rot(R):
    """The trajectory writer's matrix -> quaternion conversion (csrc/candidates.cpp quat_from_rot) in float64: (x, y, z, w)."""
    R = np.asarray(R, np.float64)
    tr = (R[0, 0] + R[1, 1]) + R[2, 2]
    if tr > 0.0:
        s = np.sqrt(tr + 1.0)
        w = 0.5 * s
        s = 0.5 / s
        x, y, z = (R[2, 1] - R[1, 2]) * s, (R[0, 2] - R[2, 0]) * s, (R[1, 0] - R[0, 1]) * s
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(((R[i, i] - R[j, j]) - R[k, k]) + 1.0)
        v = [0.0, 0.0, 0.0]
        v[i] = 0.5 * s
        s = 0.5 / s
        w = (R[k, j] - R[j, k]) * s
        v[j] = (R[j, i] + R[i, j]) * s
        v[k] = (R[k, i] + R[i, k]) * s
        x, y, z = v
    n = np.sqrt(((x * x + y * y) + z * z) + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    if w < 0.0:
        x, y, z, w = -x, -y, -z, -w
    return x, y, z, w


def quaternionf_to_rotation(w, x, y, z):
    """Eigen's Quaternionf::toRotationMatrix(), one float32 rounding per operation."""
    f = np.float32
    w, x, y, z = f(w), f(x), f(y), f(z)
    tx, ty, tz = f(2) * x, f(2) * y, f(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[f(1) - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, f(1) - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, f(1) - (txx + tyy)]], np.float32)


def node_viewpoint(pose, transform_individual_clouds):
    """ox oy oz qw qx qy qz as float32.  Flag on: Eigen::Quaternionf(0,0,0,1) is (w, x, y, z): the reference's quirk."""
    if transform_individual_clouds:
        return np.array([0, 0, 0, 0, 0, 0, 1], np.float32)
    pose = np.asarray(pose, np.float64).reshape(4, 4)
    x, y, z, w = quat_from_rot(pose[:3, :3])
    return np.array([pose[0, 3], pose[1, 3], pose[2, 3], w, x, y, z]).astype(np.float32)


def node_txt(pose, transform_individual_clouds):
    """Three rows `r0 r1 r2 t ` then `0 0 0 1` and a newline, every number as the stream prints it (:407-410)."""
    vp = node_viewpoint(pose, transform_individual_clouds)
    R = quaternionf_to_rotation(vp[3], vp[4], vp[5], vp[6])
    text = ""
    for i in range(3):
        text += "%s %s %s %s " % (fmt_g(R[i, 0]), fmt_g(R[i, 1]), fmt_g(R[i, 2]), fmt_g(vp[i]))
    return text + "0 0 0 1\n"
