"""CPU-side checks of the C-ABI boundary: the library builds for gfx950, loads without a GPU and
exports every function include/dualhyp_hip.h declares; the ctypes table covers all of them."""
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent


def _declared():
    text = (REPO / "include" / "dualhyp_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dh_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    from dualhyp_amd import _lib
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/dualhyp_hip.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)
    assert lib.dh_abi_version() == 6


def test_product_path_fails_loudly_without_gpu_tensors():
    import torch
    from dualhyp_amd import GPT, Config, _lib
    cfg = Config.from_name("parity-tiny")
    m = GPT(cfg)
    with torch.no_grad(), pytest.raises(_lib.DualHypHipError):
        m(torch.zeros(1, 4, dtype=torch.long))


def test_product_never_imports_oracle():
    for p in (REPO / "dualhyp_amd").rglob("*.py"):
        src = p.read_text()
        assert "oracle" not in re.sub(r'""".*?"""', "", src, flags=re.S).replace("# oracle", ""), p


_FAKE_S = """_ZN4testgemm_nt256w4_kernelEv:
.LBB0_1:
	;;#ASMSTART
	v_mfma_f32_16x16x32_bf16 a[0:3], v[10:13], v[20:23], a[0:3]
	;;#ASMEND
	;;#ASMSTART
	v_mfma_f32_16x16x32_bf16 a[4:7], v[10:13], v[24:27], a[4:7]
	;;#ASMEND
%s
	;;#ASMSTART
	v_mfma_f32_16x16x32_bf16 a[0:3], v[14:17], v[20:23], a[0:3]
	;;#ASMEND
	;;#ASMSTART
	s_nop 15
	s_nop 15
	;;#ASMEND
	v_accvgpr_read_b32 v1, a0
	s_endpgm
"""


def test_asm_mfma_hazard_checker(tmp_path):
    """tools/check_asm_mfma.py: the 4-wave GEMM's MFMAs are asm, invisible to the compiler's hazard recognizer; the
    checker must flag a compiler-generated accumulator read right behind the MFMA that produces it (the round-3 bug class) and a
    write right in front of the MFMA that consumes it, and accept reads behind the fence."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_asm_mfma", REPO / "tools" / "check_asm_mfma.py")
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    for body, want in (("\tv_add_u32_e32 v2, v3, v4", 0), ("\tv_accvgpr_read_b32 v1, a5", 1), ("\tv_accvgpr_write_b32 a1, v9", 1),
                       ("\tv_accvgpr_mov_b32 a2, a6", 2)):
        f = tmp_path / "k.s"
        f.write_text(_FAKE_S % body)
        assert chk.main(str(f)) == (1 if want else 0), body


def test_gemm256_has_no_asm_mfma_hazards(tmp_path):
    """The static hazard check on the assembly the regular build keeps of gemm256.hip (build() compiles that file with -save-temps=obj
    and refuses a build that fails the check; this test reads the same file, or compiles one under DUALHYP_SLOW=1 when it is missing)."""
    import os
    import subprocess
    import sys
    import __graft_entry__ as ge
    ge.build()
    s = REPO / "build" / "obj" / "gemm256-hip-amdgcn-amd-amdhsa-gfx950.s"
    if not s.exists() or s.stat().st_mtime < (ge.CSRC / "gemm256.hip").stat().st_mtime:
        if not os.environ.get("DUALHYP_SLOW"):
            pytest.skip("no current device assembly of gemm256.hip under build/obj (an older build); DUALHYP_SLOW=1 compiles one (~2 min)")
        subprocess.run([ge.HIPCC, *ge.FLAGS, "-save-temps", "-c", str(ge.CSRC / "gemm256.hip"), "-o", str(tmp_path / "g.o")], cwd=tmp_path, check=True,
                       capture_output=True)
        s = next(tmp_path.glob("*gfx950.s"))
    out = subprocess.run([sys.executable, str(REPO / "tools" / "check_asm_mfma.py"), str(s)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:]


# dh_set_tuning as it stood before the switchboard became a table (read off that function, key by key):
# key -> (default, a value the filter refuses or None when every value is taken)
_TUNING = {
    0: (1, None), 1: (5, None), 2: (1, None), 3: (1, None), 4: (0, None), 5: (0, -1), 6: (129, 0), 7: (1 << 30, 0), 8: (0, None),
    9: (0, None), 10: (0, -1), 11: (0, -1), 12: (1, None), 13: (1, None), 14: (0, 9), 15: (0, None), 16: (8, 12), 17: (0, 3),
    18: (288, 0), 19: (0, 64), 20: (0, 65), 21: (0, None), 22: (1, 3), 23: (1, None), 24: (7, None), 25: (1, None), 26: (1, None),
    27: (1, None), 28: (1, None), 29: (1, None), 30: (1, None), 31: (1, None),
}


def test_set_tuning_keys_and_value_filters():
    """Every key 0..31 takes its default value; a value outside a key's filter and a key outside the table are refused with a
    message.  Host code only: no GPU.  The defaults are set again at the end (refused values change nothing)."""
    import __graft_entry__ as ge
    ge.build()
    from dualhyp_amd import _lib
    lib = _lib.load()
    assert sorted(_TUNING) == list(range(32))
    try:
        for key, (default, refused) in _TUNING.items():
            assert lib.dh_set_tuning(key, default) == 0, f"key {key} refuses its default {default}"
            if refused is not None:
                assert lib.dh_set_tuning(key, refused) != 0, f"key {key} takes {refused}"
        for key, lo, hi in ((20, 0, 64), (22, 0, 2)):      # the two closed ranges: both ends in, one past the upper end out (above)
            assert lib.dh_set_tuning(key, lo) == 0 and lib.dh_set_tuning(key, hi) == 0
        for key, values in ((14, (0, 8, 10)), (16, (8, 16)), (17, (0, 2, 4)), (19, (0, 128, 256))):
            assert all(lib.dh_set_tuning(key, v) == 0 for v in values), key
        assert lib.dh_set_tuning(20, -1) != 0 and lib.dh_set_tuning(22, -1) != 0 and lib.dh_set_tuning(16, 0) != 0
        assert lib.dh_set_tuning(-1, 0) != 0
        assert lib.dh_set_tuning(32, 0) != 0
        assert b"32" in lib.dh_last_error()
    finally:
        for key, (default, _) in _TUNING.items():
            lib.dh_set_tuning(key, default)
