"""CPU: the comparators and the download helper of tests/gpu_support.py, which every GPU test's byte-for-byte claim goes through.  They
are pinned here so that nobody weakens all those files at once: a value comparison instead of a bytewise one fails the -0.0 case, a
download that forgets its pointers fails the free counts."""
import numpy as np
import pytest

import gpu_support as G

ROW_LIKE = np.dtype([("ix", "<i4"), ("count", "<u4"), ("x", "<f4"), ("sd", "<f4")])


def _rows(n=7):
    r = np.zeros(n, ROW_LIKE)
    r["ix"], r["count"] = np.arange(n), 3 * np.arange(n) + 1
    r["x"], r["sd"] = np.linspace(-1.0, 1.0, n), 0.25
    return r


def _fails(what, first, *args, **kw):
    """The comparison fails, and its message names `what` and the first differing index."""
    with pytest.raises(AssertionError) as e:
        G.same_records(*args, what, **kw)
    msg = str(e.value)
    assert what in msg and (first is None or "first %d" % first in msg), msg
    return msg


def test_equal_records_pass():
    rows, labels = _rows(), np.arange(7, dtype=np.uint32)
    G.same_records(rows, rows.copy(), "rows")
    G.same_records(labels, labels.copy(), "labels")
    G.same_records((rows, labels, None), (rows.copy(), labels.copy(), None), "a tuple", ("rows", "labels", "comps"))
    G.same_records(np.zeros(0, ROW_LIKE), np.zeros(0, ROW_LIKE), "no rows")
    G.same_records(labels.reshape(7, 1).repeat(3, axis=1), labels.reshape(7, 1).repeat(3, axis=1).copy(), "triangles")


def test_nans_with_identical_bits_pass():
    rows = _rows()
    rows["x"][2] = np.nan
    rows["sd"][5] = np.array([0x7FC00123], np.uint32).view(np.float32)[0]
    G.same_records(rows, rows.copy(), "rows with NaNs")


def test_one_flipped_bit_in_the_last_byte_of_the_last_record_fails():
    rows = _rows()
    other = rows.copy()
    other.view(np.uint8)[-1] ^= 0x80
    msg = _fails("flipped bit", 6, other, rows)
    assert "1 of 7" in msg
    labels = np.arange(5, dtype=np.uint32)
    other = labels.copy()
    other.view(np.uint8)[-1] ^= 1
    _fails("flipped label bit", 4, other, labels)


def test_minus_zero_is_not_plus_zero():
    rows = _rows()
    rows["x"][3] = 0.0
    other = rows.copy()
    other["x"][3] = -0.0
    assert np.array_equal(other["x"], rows["x"]), "a value comparison lets this through"
    _fails("signed zero", 3, other, rows)


def test_a_length_differing_by_one_fails():
    rows = _rows()
    assert "6 vs 7" in _fails("short by one", None, rows[:-1], rows)


def test_none_against_an_array_fails():
    rows = _rows()
    _fails("None on one side", None, (rows, None), (rows, rows), unit=("rows", "labels"))
    _fails("None on the other", None, rows, None)


def test_a_difference_in_the_second_array_only_fails():
    rows, labels = _rows(), np.arange(7, dtype=np.uint32)
    other = labels.copy()
    other[2] += 1
    other[5] += 1
    msg = _fails("second array", 2, (rows, other), (rows.copy(), labels), unit=("rows", "labels"))
    assert "2 of 7 labels" in msg


def test_planes_report_the_pixel():
    img = {"depth": np.zeros((4, 6), np.float32), "normal": np.zeros((4, 6, 3), np.float32)}
    G.same_planes(img, {k: v.copy() for k, v in img.items()}, "equal planes")
    other = {k: v.copy() for k, v in img.items()}
    other["normal"][2, 5, 1] = -0.0
    with pytest.raises(AssertionError) as e:
        G.same_planes(other, img, "a view")
    assert "a view: plane normal" in str(e.value) and "(v, u) (2, 5)" in str(e.value), str(e.value)


def test_one_differing_summary_key_fails():
    s = dict(n_rows=5, n_found=3, max_abs=0.5)
    G.same_summary(s, dict(s), ("n_rows", "n_found", "max_abs"), "summary")
    G.same_summary(s, dict(s, max_abs=0.75), ("n_rows", "n_found"), "keys that are not asked for")
    with pytest.raises(AssertionError) as e:
        G.same_summary(s, dict(s, n_found=4), ("n_rows", "n_found", "max_abs"), "one key")
    assert "one key" in str(e.value) and "n_found" in str(e.value)
    with pytest.raises(AssertionError):
        G.same_deviation((_rows(), dict.fromkeys(G.D.SUMMARY_KEYS, 0)), (_rows(), dict(dict.fromkeys(G.D.SUMMARY_KEYS, 0), pad=1)), "deviation")


class Device:
    """device_download / device_free of a handle, over a dict of byte strings."""

    def __init__(self, memory, fail_on=()):
        self.memory, self.fail_on, self.freed = memory, fail_on, []

    def device_download(self, ptr, nbytes, dtype=np.uint8):
        if ptr in self.fail_on:
            raise RuntimeError("download of %d failed" % ptr)
        return np.frombuffer(self.memory[ptr][:nbytes], dtype).copy()

    def device_free(self, ptr):
        assert ptr, "a null pointer was freed"
        self.freed.append(ptr)


def test_download_returns_the_records_or_the_empty_array():
    rows = _rows(5)
    g = Device({16: rows.tobytes(), 32: np.arange(5, dtype=np.uint32).tobytes()})
    got, labels = G.download(g, (16, 5, ROW_LIKE), (32, 5, np.uint32))
    assert got.dtype == ROW_LIKE and got.tobytes() == rows.tobytes() and labels.tolist() == [0, 1, 2, 3, 4]
    assert sorted(g.freed) == [16, 32]
    for ptr, n in ((16, 0), (0, 5), (None, 5), (0, 0)):
        g = Device({16: rows.tobytes()})
        (out,) = G.download(g, (ptr, n, ROW_LIKE))
        assert out.dtype == ROW_LIKE and out.shape == (0,), (ptr, n)
        assert g.freed == ([16] if ptr else []), (ptr, n)


def test_download_frees_every_pointer_once_also_when_it_raises():
    rows = _rows(5)
    g = Device({16: rows.tobytes(), 32: rows.tobytes(), 48: b""})
    G.download(g, (16, 5, ROW_LIKE), (0, 5, ROW_LIKE), (32, 0, ROW_LIKE), free=(48, 16, 0, None))
    assert sorted(g.freed) == [16, 32, 48]
    g = Device({16: rows.tobytes(), 32: rows.tobytes(), 48: b""}, fail_on=(16,))
    with pytest.raises(RuntimeError):
        G.download(g, (16, 5, ROW_LIKE), (32, 5, ROW_LIKE), free=(48,))
    assert sorted(g.freed) == [16, 32, 48]


def test_uploaded_frees_what_it_allocated():
    class Alloc(Device):
        def device_alloc(self, nbytes):
            self.memory[16 * (len(self.memory) + 1)] = bytes(nbytes)
            return 16 * len(self.memory)

        def device_upload(self, ptr, a):
            assert a.nbytes <= len(self.memory[ptr]), "an upload beyond its allocation"
            self.memory[ptr] = a.tobytes()

    g = Alloc({})
    with pytest.raises(RuntimeError):
        with G.uploaded(g, _rows(3), np.zeros((0, 3), np.uint32)) as (a, b):
            assert g.memory[a] == _rows(3).tobytes() and len(g.memory[b]) == 0 and g.freed == []
            raise RuntimeError("the body failed")
    assert sorted(g.freed) == [a, b]


PASS_1 = "hfpf: clean pass 1: 71159 candidates, front half on the engine's stream, replay behind the dependant-table update"
FORMS_1 = "hfpf: clean forms 1: gate tiles 4 (0 pending + 71159 new), register large, compacting no, no-wait"
PASS_2 = "hfpf: clean pass 2: 43535 candidates, front half beside the update kernel, replay fed from the registrations"
FORMS_2 = "hfpf: clean forms 2: gate tiles 1 (11786 pending + 31749 new), register small, compacting planned, waited: single 300, walked 2000, sorted, use_marks 0"


def test_clean_trace_reads_both_lines_of_a_pass():
    lines, passes = G.clean_trace("\n".join(["hfpf: shape window", PASS_1, FORMS_1, "something else", PASS_2, FORMS_2, ""]))
    assert lines == [PASS_1, FORMS_1, PASS_2, FORMS_2]
    assert passes[0] == {"pass": 1, "candidates": 71159, "beside": False, "fed": False, "gate_tiles": 4, "pending": 0, "new": 71159, "register": "large",
                         "compacting": "no", "waited": False, "single": 0, "walked": 0, "sorted": False, "use_marks": 0}
    assert passes[1] == {"pass": 2, "candidates": 43535, "beside": True, "fed": True, "gate_tiles": 1, "pending": 11786, "new": 31749, "register": "small",
                         "compacting": "planned", "waited": True, "single": 300, "walked": 2000, "sorted": True, "use_marks": 0}
    _, passes = G.clean_trace(PASS_2 + "\n" + FORMS_2.replace(", sorted,", ", unsorted,").replace("planned", "after the incremental update ran out"))
    assert not passes[0]["sorted"] and passes[0]["compacting"] == "after the incremental update ran out"
    assert G.clean_trace("") == ([], [])


@pytest.mark.parametrize("text", [PASS_1, FORMS_1, PASS_1 + "\n" + FORMS_2, PASS_1 + "\n" + FORMS_1 + " or so",
                                  PASS_1 + "\n" + FORMS_1.replace("tiles 4", "tiles 2"), PASS_1.replace("71159 candidates", "many candidates") + "\n" + FORMS_1])
def test_clean_trace_rejects_a_missing_or_garbled_line(text):
    with pytest.raises(AssertionError):
        G.clean_trace(text)
