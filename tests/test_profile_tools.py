"""The profiling tools behind profiles/r05_* (CPU): the phase-stop patch applies
to the shipped decoder source exactly once per anchor, and the VALU-mix pricing
of tools/pmc_traffic.py reads the committed issue table and prices a synthetic
record by hand; tools/kernel_isa_diff.py compares hand-written assembly by symbol."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_phase_stop_patch_applies_to_the_decoder():
    import phase_stop_patch as P
    src = open(os.path.join(ROOT, "qkd_ldpc_amd", "csrc", "decode_split.hip")).read()
    out = P.patch(src)
    # one stop point after each check phase, bit phase and syndrome test, one at the loop top
    assert out.count("QKD_STOP_POINT") == 3 + 1          # three uses + the macro definition
    assert "QKD_PMC_STOP == 0) break;" in out
    assert out.count("uint32_t pmc_ph = 0;") == 1
    # the product source itself carries no stop points
    assert "QKD_STOP_POINT" not in src


_ISA_KERNEL = """\t.text
\t.globl\tk1
k1:                                     ; @k1
; %bb.0:
\ts_load_dword s0, s[4:5], 0x0
\ts_cbranch_scc1 .LBB{n}_2
.LBB{n}_2:                               ; %exit
\tv_add_u32_e32 v0, {operand}, v0
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel k1
\t\t.amdhsa_next_free_vgpr {vgprs}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{n}:
\t.size\tk1, .Lfunc_end{n}-k1
"""


def test_kernel_isa_diff_compares_kernels_by_symbol(tmp_path):
    """Two hand-written snippets: local label counters do not count; an operand,
    a descriptor line and a kernel on one side only do."""
    import io
    import kernel_isa_diff as K

    def side(name, text):
        d = tmp_path / name
        d.mkdir()
        (d / "a.s").write_text(text)
        return K.parse_dir(str(d))

    base = side("base", _ISA_KERNEL.format(n=0, operand="s0", vgprs=1))
    moved = side("moved", _ISA_KERNEL.format(n=7, operand="s0", vgprs=1))
    out = io.StringIO()
    assert K.compare(base, moved, out) == 0
    assert "compared 1" in out.getvalue() and "instructions differ: 0" in out.getvalue()
    out = io.StringIO()
    assert K.compare(base, side("operand", _ISA_KERNEL.format(n=0, operand="s1", vgprs=1)), out) == 1
    assert "instructions differ: 1\n  k1" in out.getvalue() and "descriptor differs: 0" in out.getvalue()
    assert "+\tv_add_u32_e32 v0, s1, v0" in out.getvalue()
    out = io.StringIO()
    assert K.compare(base, side("desc", _ISA_KERNEL.format(n=0, operand="s0", vgprs=2)), out) == 1
    assert "instructions differ: 0" in out.getvalue() and "descriptor differs: 1\n  k1" in out.getvalue()
    out = io.StringIO()
    two = _ISA_KERNEL.format(n=0, operand="s0", vgprs=1) + _ISA_KERNEL.format(n=1, operand="s0", vgprs=1).replace("k1", "k2")
    assert K.compare(base, side("two", two), out) == 1
    assert "only in the change: 1\n  k2" in out.getvalue() and "only in the parent: 0" in out.getvalue()
    out = io.StringIO()
    assert K.compare(side("two_b", two), base, out) == 1
    assert "only in the parent: 1\n  k2" in out.getvalue()
    out = io.StringIO()
    twice = side("twice", _ISA_KERNEL.format(n=0, operand="s0", vgprs=1) + _ISA_KERNEL.format(n=1, operand="s0", vgprs=1))
    assert K.compare(base, twice, out) == 1
    assert "defined more than once: 1\n  k1" in out.getvalue()


def test_valu_mix_prices_the_counts_at_the_census_weighted_costs(tmp_path):
    """A synthetic census (two OTHER opcodes, a packed and a scalar FMA) and a
    synthetic record: each class at its census-weighted issue cost."""
    import json
    import pmc_traffic as T
    import valu_census as V
    cost = V.load_costs(os.path.join(ROOT, "profiles", "r06_issue_mb.txt"))
    for k in ("v_fma_f32", "v_pk_fma_f32", "v_exp_f32", "v_cndmask_b32_sgpr", "v_add_u32", "v_lshrrev_b32"):
        assert k in cost and cost[k] > 0
    census = {"v_cndmask_b32": 30.0, "v_lshrrev_b32": 10.0, "v_pk_fma_f32": 3.0, "v_fma_f32": 1.0,
              "v_add_u32": 5.0, "v_exp_f32": 2.0}
    p = tmp_path / "census.json"
    p.write_text(json.dumps({"dynamic_per_launch": census}))
    c = {"SQ_INSTS_VALU": 1000.0, "SQ_INSTS_VALU_FMA_F32": 100.0, "SQ_INSTS_VALU_TRANS_F32": 20.0,
         "SQ_INSTS_VALU_INT32": 80.0}
    cycles = 100.0                                     # per XCD-averaged GPU cycle count
    m = T.valu_mix(c, cycles, census_path=str(p), issue_path=os.path.join(ROOT, "profiles", "r06_issue_mb.txt"))
    other = (30 * cost["v_cndmask_b32_sgpr"] + 10 * cost["v_lshrrev_b32"]) / 40
    fma = (3 * cost["v_pk_fma_f32"] + 1 * cost["v_fma_f32"]) / 4
    want = 100 * fma + 20 * cost["v_exp_f32"] + 80 * cost["v_add_u32"] + (1000 - 200) * other
    assert m["simd_cycles_needed"] == pytest.approx(want, rel=1e-12)
    assert m["frac_mix"] == pytest.approx(want / (cycles * 1024), rel=1e-12)
    assert m["counts"]["OTHER"] == 800.0
    # a record without the VALU total has no mix
    assert T.valu_mix({"SQ_X": 1.0}, cycles) is None
