"""GPU: hfpf_snapshot / hfpf_restore / hfpf_save / hfpf_load (include/hfpf.h, "snapshot and restore").  A restored handle must be
indistinguishable from its source: byte-identical read-only calls, byte-identical continuations, equal contract counters."""
import os

import numpy as np
import pytest

import scenes
from gpu_support import SMALL_CAPS, contract_counters

pytestmark = pytest.mark.gpu
VIEW_K = (120.0, 120.0, 63.5, 47.5)
VIEW_Z = (0.05, 2.0)


def _grid(hfpf_mod, sc, **kw):
    return hfpf_mod.OccupancyGrid(resolution=sc.resolution, bbox=sc.bbox, **dict(SMALL_CAPS, **kw))


def _scene(n=6, **kw):
    return scenes.Scene(n, 128, 96, 0.001, fx=615.0, clean_every=3, **kw)


# ---- 1. read-only identity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [False, True], ids=["plain", "colour"])
def test_read_only_identity(hfpf_mod, synth_mod, color):
    sc = _scene(7)
    with _grid(hfpf_mod, sc, fuse_color=color, binned_update=True, frame_width=128) as src:
        scenes.run(src, sc, "integrate")  # ends with a clean
        blob = src.snapshot()
        info = hfpf_mod.snapshot_info(blob)
        assert info["total_bytes"] == len(blob) and info["max_log_points"] == SMALL_CAPS["max_log_points"]
        assert info["voxels_with_normal"] > 1000 and info["frames_integrated"] == 7 and info["next_frame_id"] == 7
        assert info["max_bricks"] <= 30000 and info["max_normals"] <= 1 << 19
        # the other update form, other pool sizes, no tiling hint
        with _grid(hfpf_mod, sc, fuse_color=color, binned_update=False, frame_width=0, max_bricks=30000, max_normals=1 << 19) as dst:
            dst.restore(blob)
            cloud = sc.frame(2)
            lay = sc.layout
            for what, call in (
                    ("extract", lambda g: g.extract()),
                    ("extract_filtered", lambda g: g.extract_filtered(min_count=5.0)),
                    ("occupied", lambda g: g.occupied()),
                    ("dirty", lambda g: np.array([g.state_changed])),
                    ("render", lambda g: np.concatenate([v.reshape(-1).view(np.uint8) for _, v in sorted(
                        g.render(sc.poses[0], VIEW_K, 128, 96, z_range=VIEW_Z, splat_radius=1).items())])),
                    ("query", lambda g: np.concatenate([a.view(np.uint8).reshape(-1) for a in g.query(cloud, sc.poses[2], layout=lay, radius=1)])),
                    ("mesh", lambda g: np.concatenate([a.reshape(-1).view(np.uint8) for a in g.extract_mesh(radius=2)])),
                    ("raycast_view", lambda g: g.raycast_view(sc.poses[0], VIEW_K, 128, 96, t_range=VIEW_Z)),
            ):
                a, b = call(src), call(dst)
                assert len(a) > 0, what
                assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), "%s differs after restore" % what
            rows = dst.extract()
            assert len(rows) > 1000 and (not color or (rows["rgb"][rows["count"] > 0] != 0).any())
            assert (dst.render(sc.poses[0], VIEW_K, 128, 96, z_range=VIEW_Z, splat_radius=1)["count"] > 0).any()
            assert contract_counters(src) == contract_counters(dst)


# ---- 2. continuation under random schedules -------------------------------------------------------------------------------
def _script(rng, n_frames):  # tests/test_gpu_random_schedules.py
    ops, f = [], 0
    while f < n_frames:
        r = rng.random()
        if r < 0.55:
            run = int(rng.integers(1, 4))
            for _ in range(min(run, n_frames - f)):
                ops.append(("integrate", f))
                f += 1
        elif r < 0.80:
            ops.append(("clean",))
            if rng.random() < 0.2:
                ops.append(("clean",))  # a second pass with nothing new is a no-op for the rows
        elif r < 0.92:
            ops.append(("extract",))
        else:
            ops.append(("clear",))
    ops += [("clean",), ("extract",)]
    return ops


FORCED = ["first", "after_integrate", "after_clean", "after_clear"]  # seed % 4 picks where the second handoff is forced


def _with_handoffs(rng, ops, forced):
    ops = list(ops)
    ops.insert(int(rng.integers(0, len(ops) + 1)), ("handoff",))
    if forced == "first":
        ops.insert(0, ("handoff",))
        return ops
    kind = forced[len("after_"):]
    where = [i for i, op in enumerate(ops) if op[0] == kind and (i + 1 == len(ops) or ops[i + 1][0] != "handoff")]
    if not where:  # the script holds no such op (no clear drawn): make one, then hand off
        at = int(rng.integers(0, len(ops)))
        ops.insert(at, (kind,))
        where = [at]
    ops.insert(where[int(rng.integers(0, len(where)))] + 1, ("handoff",))
    return ops


N_SEEDS = int(os.environ.get("HFPF_SOAK_SEEDS", "12"))


@pytest.mark.parametrize("seed", list(range(N_SEEDS)))
def test_continuation_random_schedule(oracle_mod, hfpf_mod, synth_mod, seed):
    rng = np.random.default_rng(4000 + seed)
    res, fx, W, H = [(0.001, 615.0, 128, 96), (0.005, 0.0, 128, 96), (0.002, 615.0, 160, 120)][seed % 3]
    cfg = {}
    if rng.random() < 0.3:
        cfg["K"] = int(rng.integers(1, 5))
    if rng.random() < 0.3:
        cfg["gate"] = int(rng.integers(12, 30))
    if rng.random() < 0.2:
        cfg["pcl_shifted_cov"] = True
    sc = scenes.Scene(int(rng.integers(5, 10)), W, H, res, fx=fx, seed=0xF051 + seed, pose_seed=0x5E3 + seed)
    ops = _with_handoffs(rng, _script(rng, sc.n_frames), FORCED[seed % 4])
    assert sum(op[0] == "handoff" for op in ops) >= 2
    fw = W if (seed // 2) % 2 else 0

    def make(flip=False):  # a handoff also alternates the update form of the new handle
        return hfpf_mod.OccupancyGrid(resolution=res, bbox=sc.bbox, binned_update=bool(seed % 2) != flip, frame_width=fw, **cfg, **SMALL_CAPS)

    og = oracle_mod.OracleGrid(resolution=res, bbox=sc.bbox, **cfg)
    plain, handed = make(), make()
    n_checked = n_handoffs = 0
    try:
        for op in ops:
            if op[0] == "integrate":
                buf = sc.frame(op[1])
                og.capture(buf, sc.poses[op[1]])
                plain.integrate(buf, sc.poses[op[1]])
                handed.integrate(buf, sc.poses[op[1]])
            elif op[0] == "clean":
                og.clean()
                plain.clean()
                handed.clean()
                assert plain.state_changed == og.is_dirty() and handed.state_changed == og.is_dirty()
            elif op[0] == "extract":
                ref, a, b = og.extract(), plain.extract(), handed.extract()
                scenes.compare_rows(ref, a)
                assert a.tobytes() == b.tobytes(), "rows differ after %d handoff(s)" % n_handoffs
                n_checked += 1
            elif op[0] == "clear":
                og.clear()
                plain.clear()
                handed.clear()
                assert len(handed.extract()) == 0
            else:  # snapshot, destroy, create, restore
                blob = handed.snapshot()
                dirty = handed.state_changed
                handed.close()
                n_handoffs += 1
                handed = make(flip=bool(n_handoffs % 2))
                handed.restore(blob)
                assert handed.state_changed == dirty
        assert np.array_equal(og.occupied(), plain.occupied())
        assert plain.occupied().tobytes() == handed.occupied().tobytes()
        assert contract_counters(plain) == contract_counters(handed)
    finally:
        plain.close()
        handed.close()
        og.close()
    assert n_checked >= 1 and n_handoffs >= 2


# ---- 3. waiting host frames ---------------------------------------------------------------------------------------------
def test_waiting_host_frames_are_in_the_snapshot(hfpf_mod, synth_mod):
    sc = _scene(6)
    with _grid(hfpf_mod, sc) as a, _grid(hfpf_mod, sc) as b:
        for f in range(sc.n_frames):  # back to back through the host path: frames may still wait for their launch
            a.integrate(sc.frame(f), sc.poses[f])
        blob = a.snapshot()  # at once
        b.restore(blob)
        assert hfpf_mod.snapshot_info(blob)["frames_integrated"] == sc.n_frames
        for g in (a, b):
            g.clean()
        ra, rb = a.extract(), b.extract()
        assert len(ra) > 1000 and ra.tobytes() == rb.tobytes()
        assert a.occupied().tobytes() == b.occupied().tobytes() and contract_counters(a) == contract_counters(b)


# ---- 4. files ------------------------------------------------------------------------------------------------------------
def test_files(hfpf_mod, synth_mod, tmp_path):
    sc = _scene(6)
    path = str(tmp_path / "session.hfpf")
    with _grid(hfpf_mod, sc) as src:
        rows = scenes.run(src, sc, "integrate").copy()
        src.integrate(sc.frame(0), sc.poses[0])  # dirty: a frame since the last clean
        src.save(path)
        blob = src.snapshot().tobytes()
        assert open(path, "rb").read() == blob
        with _grid(hfpf_mod, sc) as by_file, _grid(hfpf_mod, sc) as by_blob:
            by_file.load(path)
            by_blob.restore(blob)
            for g in (src, by_file, by_blob):
                g.clean()
            want = src.extract()
            assert len(want) >= len(rows) and want.tobytes() == by_file.extract().tobytes() == by_blob.extract().tobytes()
            assert contract_counters(by_file) == contract_counters(by_blob) == contract_counters(src)
    # damaged and missing files are refused and leave the target as it was
    half, flipped = str(tmp_path / "half.hfpf"), str(tmp_path / "flipped.hfpf")
    open(half, "wb").write(blob[:len(blob) // 2])
    bad = bytearray(blob)
    bad[hfpf_mod.SNAPSHOT_HEADER_BYTES + (len(blob) - hfpf_mod.SNAPSHOT_HEADER_BYTES) // 3] ^= 0x10  # one payload byte
    open(flipped, "wb").write(bytes(bad))
    sc5 = scenes.Scene(2, 128, 96, 0.001, fx=615.0)
    with _grid(hfpf_mod, sc5) as g:
        had = scenes.run(g, sc5, "integrate").copy()
        assert len(had) > 100
        for p, code in ((half, -6), (flipped, -2), (str(tmp_path / "missing.hfpf"), -6)):  # IO: not readable in full; BAD_ARG: checksum
            with pytest.raises(hfpf_mod.HfpfError) as e:
                g.load(p)
            assert e.value.code == code, p
            assert g.extract().tobytes() == had.tobytes()
        with pytest.raises(hfpf_mod.HfpfError) as e:
            g.restore(bytes(bad))
        assert e.value.code == -2
        with pytest.raises(hfpf_mod.HfpfError) as e:
            g.restore(blob[:len(blob) // 2])  # shorter than its header says
        assert e.value.code == -2
        with pytest.raises(hfpf_mod.HfpfError) as e:
            g.save(str(tmp_path / "no_such_dir" / "x.hfpf"))
        assert e.value.code == -6
        assert g.extract().tobytes() == had.tobytes()


# ---- 5. mismatch ---------------------------------------------------------------------------------------------------------
def test_mismatch_is_refused_and_the_target_lives_on(hfpf_mod, synth_mod):
    sc = _scene(6)
    with _grid(hfpf_mod, sc) as src:
        scenes.run(src, sc, "integrate")
        blob = src.snapshot()
        n_records = src.counters()["voxels_with_normal"]
    assert n_records > 2048
    bb = list(sc.bbox)
    bb[1] += 0.25
    base = dict(resolution=sc.resolution, bbox=sc.bbox)
    cases = [(dict(resolution=0.002), -1), (dict(bbox=tuple(bb)), -1), (dict(K=2), -1), (dict(fuse_color=True), -1),
             (dict(max_log_points=2 << 20), -1), (dict(max_normals=2048), -3)]
    for kw, code in cases:
        # the target's own session: 768 points for the handle with 2048 records, three frames otherwise
        own = scenes.Scene(2, 32, 24, 0.001, fx=615.0) if code == -3 else scenes.Scene(3, 128, 96, 0.001, fx=615.0)
        with hfpf_mod.OccupancyGrid(**dict(base, **dict(SMALL_CAPS, **kw))) as g:
            g.integrate(own.frame(0), own.poses[0])
            g.clean()
            had, had_occ = g.extract().copy(), g.occupied()
            assert len(had_occ) > 0
            with pytest.raises(hfpf_mod.HfpfError) as e:
                g.restore(blob)
            assert e.value.code == code, kw
            assert g.extract().tobytes() == had.tobytes() and g.occupied().tobytes() == had_occ.tobytes(), kw
            g.integrate(own.frame(1), own.poses[1])  # and accepts further frames
            g.clean()
            g.sync()
            assert g.counters()["frames_integrated"] == 2 and len(g.occupied()) >= len(had_occ)


# ---- 6. canonical bytes ----------------------------------------------------------------------------------------------------
def test_canonical_bytes(hfpf_mod, synth_mod, monkeypatch):
    sc = _scene(6)
    H = hfpf_mod.SNAPSHOT_HEADER_BYTES
    with _grid(hfpf_mod, sc) as g:
        empty = g.snapshot().tobytes()
        assert len(empty) < 64 << 10
        scenes.run(g, sc, "integrate")
        g.integrate(sc.frame(1), sc.poses[1])
        one, two = g.snapshot().tobytes(), g.snapshot().tobytes()
        assert one == two
        # a staging window far below the payload: packed and downloaded in groups, same bytes
        monkeypatch.setenv("HFPF_TEST_SNAPSHOT_WINDOW", str(1 << 18))
        assert len(one) > 1 << 20 and g.snapshot().tobytes() == one
        with _grid(hfpf_mod, sc) as w:
            w.restore(one)  # ... and uploaded and unpacked in groups
            monkeypatch.delenv("HFPF_TEST_SNAPSHOT_WINDOW")
            assert w.snapshot().tobytes() == one
        with _grid(hfpf_mod, sc, max_bricks=40000, binned_update=False) as r:
            r.restore(one)
            again = r.snapshot().tobytes()
        # no header field describes the handle (only needed capacities are stored), except the source's flags word
        i1, i2 = hfpf_mod.snapshot_info(one), hfpf_mod.snapshot_info(again)
        assert i1["payload_checksum"] == i2["payload_checksum"] and one[H:] == again[H:]
        assert {k for k in i1 if i1[k] != i2[k]} <= {"flags"}
    with _grid(hfpf_mod, sc, max_bricks=4 * SMALL_CAPS["max_bricks"], max_normals=4 * SMALL_CAPS["max_normals"]) as big:
        scenes.run(big, sc, "integrate")
        big.integrate(sc.frame(1), sc.poses[1])
        assert len(big.snapshot()) == len(one)
    with _grid(hfpf_mod, sc) as e:
        e.restore(empty)
        assert len(e.extract()) == 0 and len(e.occupied()) == 0 and e.snapshot().tobytes() == empty
        e.clear()
        assert e.snapshot().tobytes()[H:] == empty[H:]  # after a clear: the empty payload again (the header says dirty)


# ---- 7. state rules -------------------------------------------------------------------------------------------------------
def test_state_rules(hfpf_mod, synth_mod):
    sc = scenes.Scene(2, 160, 120, 0.001, fx=615.0)
    tiny = scenes.Scene(1, 32, 24, 0.001, fx=615.0)  # 768 points: fits a handle with 256 records (1024 occupied cells)
    with _grid(hfpf_mod, sc) as good:
        want = scenes.run(good, sc, "integrate").copy()
        blob = good.snapshot().tobytes()
    with _grid(hfpf_mod, tiny) as t:
        t.integrate(tiny.frame(0), tiny.poses[0])
        tiny_blob = t.snapshot().tobytes()  # dirty, no clean yet
        tiny_occ = t.occupied()
    assert len(tiny_occ) > 0 and hfpf_mod.snapshot_info(tiny_blob)["max_normals"] <= 256
    with _grid(hfpf_mod, sc, max_normals=256) as g:  # a legitimately too small pool in a clean pass (tests/test_gpu_multirank.py)
        g.integrate(sc.frame(0), sc.poses[0])
        with pytest.raises(hfpf_mod.HfpfError) as e:
            g.clean()
        assert e.value.code == -3
        with pytest.raises(hfpf_mod.HfpfError) as e:
            g.snapshot()
        assert e.value.code == -5 and "hfpf_clear" in str(e.value)
        with pytest.raises(hfpf_mod.HfpfError) as e:
            g.restore(blob)  # the large session does not fit: refused on the host, the handle is still poisoned
        assert e.value.code == -3
        with pytest.raises(hfpf_mod.HfpfError) as e:
            g.extract()
        assert e.value.code == -5
        g.restore(tiny_blob)  # restore begins with a clear: the handle works again
        assert g.state_changed and len(g.extract()) == 0
        assert g.occupied().tobytes() == tiny_occ.tobytes()
        assert g.snapshot().tobytes()[hfpf_mod.SNAPSHOT_HEADER_BYTES:] == tiny_blob[hfpf_mod.SNAPSHOT_HEADER_BYTES:]
    with _grid(hfpf_mod, sc) as g:
        g.integrate(sc.frame(0), sc.poses[0])
        g.epoch_export()
        for call in (g.snapshot, lambda: g.restore(blob)):
            with pytest.raises(hfpf_mod.HfpfError) as e:
                call()
            assert e.value.code == -5
    with _grid(hfpf_mod, sc) as g:
        g.restore(blob)
        assert g.extract().tobytes() == want.tobytes()


# ---- 8. node shell ---------------------------------------------------------------------------------------------------------
def test_node_session_handoff(hfpf_mod, synth_mod, tmp_path):
    import hfpf_node
    sc = scenes.Scene(6, 128, 96, 0.001, fx=615.0)
    dirs = [tmp_path / "whole", tmp_path / "first", tmp_path / "second"]
    for d in dirs:
        d.mkdir()
    session = str(tmp_path / "session.hfpf")

    def node(d):
        n = hfpf_node.FusionNode(bounding_box=list(sc.bbox), directory_name=str(d), tf_lookup=lambda t, s: sc.poses[int(s)],
                                 resolution=sc.resolution, final_clean_on_process=True, **SMALL_CAPS)
        n.start()
        return n

    def feed(n, frames):
        for f in frames:
            assert n.publish(sc.frame(f), 1, sc.W * sc.H, frame_id=str(f)) == 1
            if f % 2 == 1:
                n.clean_now()

    with node(dirs[0]) as whole:
        feed(whole, range(6))
        assert whole.process()[1]
    with node(dirs[1]) as first:
        feed(first, range(3))
        first.save_session(session)
    with node(dirs[2]) as second:
        second.stop()
        second.load_session(session)
        assert second.stats()["started"] == 0  # load keeps the node's started / stopped state
        second.start()
        feed(second, range(3, 6))
        assert second.process()[1]
        with pytest.raises(hfpf_mod.HfpfError) as e:
            second.load_session(str(tmp_path / "missing.hfpf"))
        assert e.value.code == -6
    for name in ("test_cloud.pcd", "meta.csv"):
        a, b = (dirs[0] / name).read_bytes(), (dirs[2] / name).read_bytes()
        assert len(a) > 1000 and a == b, name
