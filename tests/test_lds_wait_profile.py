"""scripts/lds_wait_profile.py on a hand-written loop: which operation each wait releases, the issue cycles between,
the next consumer, and the single-wave stall model."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ASM = """
\t.text
_Z4toy_kernelPf:                        ; @_Z4toy_kernelPf
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
\tds_read_b128 v[10:13], v1
\ts_waitcnt lgkmcnt(0)
\tv_mfma_f32_16x16x32_bf16 v[20:23], v[10:13], v[30:33], v[20:23]
\tds_read_b128 v[10:13], v1 offset:1024
\tds_read_b128 v[14:17], v1 offset:2048
\tv_add_f32_e32 v2, v3, v4
\tv_exp_f32_e32 v5, v2
\ts_waitcnt lgkmcnt(1)
\tv_mfma_f32_16x16x32_bf16 v[20:23], v[10:13], v[30:33], v[20:23]
\ts_waitcnt lgkmcnt(0)
\tv_add_f32_e32 v6, v14, v5
\ts_add_i32 s2, s2, -1
\ts_cmp_lg_u32 s2, 0
\ts_cbranch_scc1 .LBB0_1
\ts_endpgm
.Lfunc_end0:
"""


def test_wait_table_of_a_toy_loop(tmp_path):
    path = tmp_path / "toy.s"
    path.write_text(ASM)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "lds_wait_profile.py"), str(path), "toy_kernel",
                          "--latency", "64"], capture_output=True, text=True, check=True).stdout
    rows = [l.split() for l in out.splitlines() if l.strip() and l.split()[0].isdigit()]
    assert len(rows) == 3, out
    # wait 1: lgkmcnt(0) right behind its read, nothing between, consumer an MFMA, the whole latency exposed
    assert rows[0][1] == "0" and rows[0][2] == "ds_read_b128" and rows[0][-1] == "MFMA"
    assert [int(x) for x in rows[0][5:9]] == [1, 0, 0, 64]
    # wait 2: lgkmcnt(1) releases the first of two reads: the second read, a VALU (4) and a transcendental (8) between;
    # the clock stands 8 (wait 1's MFMA) + 12 behind the read's issue at clock 72 -> back at 136, reached at 84
    assert rows[1][1] == "1" and rows[1][4] == "v[10:13]" and rows[1][-1] == "MFMA"
    assert [int(x) for x in rows[1][5:9]] == [1, 3, 12, 52]
    # wait 3: the second read, behind the first one's wait; its consumer is a VALU
    assert rows[2][1] == "0" and rows[2][4] == "v[14:17]" and "v_add_f32_e32" in rows[2][-2]
    assert [int(x) for x in rows[2][5:9]] == [1, 4, 20, 0]
    assert "waits on lgkmcnt: 3 (lgkmcnt(0): 2, lgkmcnt(1): 1)" in out
    assert "exposed sites (LDS read -> wait -> MFMA, fewer than 64 issue cycles between): 2, of them at lgkmcnt(0): 1" in out
    assert "modelled stall" in out and ": 116 cycles, before an MFMA: 116" in out
