"""Stream inputs without a GPU: ``-`` without ``-r`` is refused as PyMaSC refuses an unseekable input (handler/calc.py:81,
pymasc.py:199-201) before a byte of it is read, ``-`` is named once and read by one process, and the stream predicate."""
import os
import subprocess
import sys

from pymasc_amd import cli, inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(argv, stdin, timeout=300):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    return subprocess.run([sys.executable, "-m", "pymasc_amd"] + argv, stdin=stdin, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, env=env, timeout=timeout)


def test_stdin_without_read_length_is_skipped_unread(tmp_path):
    r, w = os.pipe()
    payload = b"\x1f\x8b\x08\x04" + b"\0" * 60
    os.write(w, payload)
    try:
        p = _child(["-", "-d", "300", "-o", str(tmp_path / "out"), "--skip-plots"], r)
        os.close(w)
        w = None
        left = os.read(r, 1 << 16)
    finally:
        os.close(r)
        if w is not None:
            os.close(w)
    assert p.returncode == 1, p.stderr
    assert "Cannot execute read length checking for unseekable input." in p.stderr
    assert "If your input can't reread, specify read length using `-r` option." in p.stderr
    assert "No input file could be run." in p.stderr
    assert "Failed to open file '-'" not in p.stderr
    assert left == payload                # nothing of the stream was read


def test_stdin_twice_or_with_ranks_is_an_argument_error(tmp_path, monkeypatch):
    from pymasc_amd import launch
    monkeypatch.setattr(launch, "spawn_ranks", lambda *a, **k: (_ for _ in ()).throw(AssertionError("spawned")))
    assert cli.main(["-", "-r", "36", "-p", "2", "-o", str(tmp_path)]) == 2
    assert cli.main(["-", "-", "-r", "36", "-o", str(tmp_path)]) == 2
    assert not any(tmp_path.iterdir())


def test_stream_predicate(tmp_path):
    fifo = tmp_path / "fifo"
    os.mkfifo(fifo)
    reg = tmp_path / "x.bam"
    reg.write_bytes(b"x")
    assert inputs.is_stream("-")
    assert inputs.is_stream(str(fifo))
    assert not inputs.is_stream(str(reg))
    assert not inputs.is_stream(str(tmp_path / "missing.bam"))
