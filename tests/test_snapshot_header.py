"""CPU: hfpf_snapshot_info and hfpf_config_from_snapshot are host code (no handle, no GPU).  A header is written here by hand from
the layout csrc/snapshot.hpp documents (SnapHeader) with a restatement of its checksum, so the test also pins the format."""
import ctypes as C
import struct

import numpy as np
import pytest

HEADER = 4096
MASK = (1 << 64) - 1


def _checksum(data):
    """snap_checksum of csrc/snapshot.hpp: four multiply-xorshift lanes over the 8-byte words, folded with the length."""
    mul = 0x9E3779B97F4A7C15
    lanes = [0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89]
    words = struct.unpack("<%dQ" % (len(data) // 8), data)
    for i in range(0, len(words) - 3, 4):
        for j in range(4):
            v = ((lanes[j] ^ words[i + j]) * mul) & MASK
            lanes[j] = v ^ (v >> 29)
    r = len(data)
    for v in lanes:
        r = ((r ^ v) * mul) & MASK
        r ^= r >> 32
    return r


FIELDS = dict(resolution=0.0025, flags=3, bbox=(-0.25, 0.5, -1.0, 1.0, 0.125, 2.0), k=2, K=4, gate=17, cylinder_radius=0.002,
              ball_radius=0.02, z_clip_min=0.3, z_clip_max=0.7, max_bricks=1234, max_log_points=1 << 20, max_normals=56789,
              max_frames=77, frames_integrated=70, clean_passes=9, next_frame_id=71, voxels_occupied=400000, voxels_with_normal=56000)


def _header(magic=b"HFPFSNAP", version=1, header_bytes=HEADER, payload_bytes=512, seal=True):
    f = FIELDS
    h = bytearray(HEADER)
    struct.pack_into("<8sIIQQQQQ", h, 0, magic, version, header_bytes, 0x1234, HEADER + payload_bytes, payload_bytes, 0xABCDEF, 0)
    struct.pack_into("<fI6d4i4d", h, 56, f["resolution"], f["flags"], *f["bbox"], f["k"], f["K"], f["gate"], 0, f["cylinder_radius"],
                     f["ball_radius"], f["z_clip_min"], f["z_clip_max"])
    struct.pack_into("<9Q", h, 160, f["max_bricks"], f["max_log_points"], f["max_normals"], f["max_frames"], f["frames_integrated"],
                     f["clean_passes"], f["next_frame_id"], f["voxels_occupied"], f["voxels_with_normal"])
    if seal:
        struct.pack_into("<Q", h, 48, _checksum(bytes(h)))
    return bytes(h)


def test_info_struct_has_the_asserted_size(hfpf_mod):
    assert C.sizeof(hfpf_mod.SnapshotInfo) == 248  # static_assert in csrc/snapshot.hpp
    assert hfpf_mod.SNAPSHOT_HEADER_BYTES == HEADER


def test_info_reads_a_header_alone(hfpf_mod):
    info = hfpf_mod.snapshot_info(_header())  # exactly the header's bytes: the payload is not needed
    for k, v in FIELDS.items():
        if k == "resolution":
            assert np.float32(info[k]) == np.float32(v)
        else:
            assert info[k] == v, k
    assert info["format_version"] == 1 and info["layout_tag"] == 0x1234
    assert info["total_bytes"] == HEADER + 512 and info["payload_bytes"] == 512 and info["payload_checksum"] == 0xABCDEF
    assert hfpf_mod.snapshot_info(_header() + b"\0" * 100)["max_frames"] == 77  # more bytes than the header are fine


def _raw_info(hfpf_mod, blob, nbytes, struct_size=None):
    """The C call itself, with a canary-filled output struct: (status, output bytes)."""
    s = hfpf_mod.SnapshotInfo()
    C.memset(C.byref(s), 0xA5, C.sizeof(s))
    s.struct_size = C.sizeof(s) if struct_size is None else struct_size
    before = bytes(s)
    buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(blob or b"\0") if blob is not None else None
    rc = hfpf_mod.lib().hfpf_snapshot_info(buf, nbytes, C.byref(s))
    return rc, before, bytes(s)


@pytest.mark.parametrize("case", ["null", "zero_bytes", "short", "magic", "struct_size", "version", "header_bytes", "checksum"])
def test_info_rejects_and_writes_nothing(hfpf_mod, case):
    good = _header()
    blob, nbytes, ss = good, len(good), None
    if case == "null":
        blob = None
    elif case == "zero_bytes":
        nbytes = 0
    elif case == "short":
        nbytes = HEADER - 1
    elif case == "magic":
        blob = _header(magic=b"HFPFSNAQ")
    elif case == "struct_size":
        ss = 240
    elif case == "version":
        blob = _header(version=2)
    elif case == "header_bytes":
        blob = _header(header_bytes=8192)
    elif case == "checksum":
        blob = bytearray(good)
        blob[200] ^= 1  # clean_passes
        blob = bytes(blob)
    rc, before, after = _raw_info(hfpf_mod, blob, nbytes, ss)
    assert rc == -2  # HFPF_ERR_BAD_ARG
    assert after == before, "a rejected call wrote into the output struct"
    s = hfpf_mod.SnapshotInfo()
    s.struct_size = C.sizeof(s)
    assert hfpf_mod.lib().hfpf_snapshot_info((C.c_uint8 * HEADER).from_buffer_copy(good), HEADER, None) == -2  # NULL out


def test_python_wrapper_raises(hfpf_mod):
    with pytest.raises(hfpf_mod.HfpfError) as e:
        hfpf_mod.snapshot_info(b"\0" * HEADER)
    assert e.value.code == -2
    with pytest.raises(hfpf_mod.HfpfError):
        hfpf_mod.snapshot_info(b"")


def test_config_from_snapshot_field_by_field(hfpf_mod):
    info = dict(FIELDS)  # hand-filled
    cfg = hfpf_mod.config_from_snapshot(info)
    d = hfpf_mod.default_config()
    assert cfg.struct_size == C.sizeof(hfpf_mod.Config)
    assert np.float32(cfg.resolution) == np.float32(FIELDS["resolution"])
    assert tuple(cfg.bbox) == FIELDS["bbox"]
    assert (cfg.k, cfg.K, cfg.gate) == (2, 4, 17)
    assert (cfg.cylinder_radius, cfg.ball_radius, cfg.z_clip_min, cfg.z_clip_max) == (0.002, 0.02, 0.3, 0.7)
    assert cfg.flags == 3  # colour fusion + shifted covariance
    assert (cfg.max_bricks, cfg.max_log_points, cfg.max_normals, cfg.max_frames) == (1234, 1 << 20, 56789, 77)
    # device and scheduling hints stay at their defaults
    assert (cfg.device, cfg.frame_width, cfg.reserved0, cfg.max_call_points) == (d.device, d.frame_width, d.reserved0, d.max_call_points)
    info["flags"] = 3 | hfpf_mod.FLAG_DIRECT_UPDATE  # the update form of the source is no property of the session
    assert hfpf_mod.config_from_snapshot(info).flags == 3
    # the C call refuses NULL and a wrong struct_size
    L = hfpf_mod.lib()
    s = hfpf_mod._snapshot_info_struct(FIELDS)
    c = hfpf_mod.Config()
    assert L.hfpf_config_from_snapshot(None, C.byref(c)) == -2 and L.hfpf_config_from_snapshot(C.byref(s), None) == -2
    s.struct_size = 8
    assert L.hfpf_config_from_snapshot(C.byref(s), C.byref(c)) == -2
