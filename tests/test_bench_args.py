"""CPU: bench.py refuses a measurement a plain run does not make before it touches the GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_write_dir_needs_full(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--write-dir", str(tmp_path / "w")],
                         capture_output=True, timeout=120, cwd=ROOT)
    assert out.returncode == 2 and "--full" in out.stderr.decode()
    assert out.stdout.decode().strip() == "" and not os.path.exists(str(tmp_path / "w"))
