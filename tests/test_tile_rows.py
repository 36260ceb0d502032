"""The edge-message kernel computes a row's endpoints from its 16-byte tile descriptor (flowmol_amd/csrc/fm_tile_desc.h) instead of loading them from
e_src / e_dst / e_pair / node_first_edge.  The helper is plain C++: tests/tile_rows_check.cpp compares it, on the host, with the definition of the edge
order as fm_k_batch_setup writes it (`/` and `%`): every n in 2 .. 300 at tile heights 16 / 32 / 64, every tile and row; n = 4097, 23,169 and 23,170 (the
largest molecule a batch can hold) on the first, middle and last three tiles; node and edge offsets small and at the limits of a bound batch; the
reciprocal exact and two ulp off to either side (the kernels pass the hardware's approximate reciprocal)."""
import shutil
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
SRC = HERE / 'tile_rows_check.cpp'


def _cxx():
    for c in ('/opt/rocm/lib/llvm/bin/clang++', shutil.which('clang++'), shutil.which('g++'), shutil.which('c++')):
        if c and Path(c).exists():
            return c
    pytest.skip('no host C++ compiler')


def _build_and_run(tmp_path, flags, args):
    exe = tmp_path / 'tile_rows_check'
    r = subprocess.run([_cxx(), '-std=c++17', *flags, str(SRC), '-o', str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and any(f.startswith('-fsanitize') for f in flags) and any(w in r.stderr for w in ('asan', 'ubsan', 'sanitizer')):
        pytest.skip('this host compiler has no sanitizer runtime: ' + r.stderr.strip().splitlines()[-1])      # a missing runtime library, not an error in the source (the plain build above compiles it)
    assert r.returncode == 0, r.stderr
    return subprocess.run([str(exe), *args], capture_output=True, text=True)


def test_row_endpoints_from_the_descriptor_match_the_setup_kernels_formulas(tmp_path):
    r = _build_and_run(tmp_path, ['-O2', '-ffp-contract=off'], [])
    assert r.returncode == 0, r.stdout + r.stderr
    rows = int(r.stdout.split('rows checked:')[1].split(',')[0])
    assert rows > 3 * 3 * sum(n * (n - 1) for n in range(2, 301))      # every row of every small molecule at three heights and three reciprocals, plus the large ones


def test_row_helper_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same program as a stand-alone sanitizer build: no signed overflow or out-of-range shift in the packing or in the row arithmetic at the limits."""
    r = _build_and_run(tmp_path, ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], ['quick'])
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'runtime error' not in r.stderr and 'mismatches: 0' in r.stdout
