"""not gpu: static checks of the forward's identity route (kprn_amd/csrc/lstm_fused_fwd.hip fwd_body IDENT) on the ISA hipcc emits
(hipcc -S needs no GPU), with scripts/check_mfma_hazards.py like tests/test_hazards.py:
  * the IDENT instantiations exist: the 64-row kernels with and without the training saves, the dual kernel (and the 16-row ones);
  * each has no unprotected MFMA hazard, at most 8 spilled registers, and hot blocks (>= 60 MFMAs) that write nothing to scratch and reload at most one register;
  * a slot of an IDENT instantiation issues FEWER MFMAs than its full-row twin, in the ratio the design says: per recurrent slot (8 units) layer 0's four input
    halves have three k-groups instead of four, 4 x 16 MFMAs less -- counted from what the compiler emitted, the slot bodies matched one to one."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import check_mfma_hazards as chk  # noqa: E402

SRC = os.path.join(ROOT, "kprn_amd", "csrc", "lstm_fused_fwd.hip")
# k_lstm_fwd<L, SAVE, IDENT, NMT>, k_lstm_fwd_dual<L, IDENT, NMT>
SINGLE = r"_ZN5fused\d+k_lstm_fwdILi2ELb%dELb%dELi%dEEEv\w+"
DUAL = r"_ZN5fused\d+k_lstm_fwd_dualILi2ELb%dELi%dEEEv\w+"


def _bodies(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"\n(_ZN5fused\d+k_lstm_fwd\w+):[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)}


def _find(bodies, pattern):
    hit = [k for k in bodies if re.fullmatch(pattern, k)]
    assert len(hit) == 1, (pattern, sorted(bodies))
    return hit[0]


def _mfma_per_block(body):
    return [len(re.findall(r"\bv_mfma", b)) for b in re.split(r"\n\.LBB\d+_\d+:", body)]


def _twins(bodies):
    """(IDENT symbol, full-row symbol, 64-row tiles) of every instantiation pair"""
    out = []
    for nmt in (4, 1):
        for save in (1, 0):
            out.append((_find(bodies, SINGLE % (save, 1, nmt)), _find(bodies, SINGLE % (save, 0, nmt)), nmt == 4))
        out.append((_find(bodies, DUAL % (1, nmt)), _find(bodies, DUAL % (0, nmt)), nmt == 4))
    return out


def test_ident_instantiations_exist_and_are_clean():
    text = chk.compile_isa(SRC)
    bodies = _bodies(text)
    res = chk.kernel_resources(text)
    assert chk.check_text(text, os.path.basename(SRC)) == 0
    for ident, _, big in _twins(bodies):
        v = res[ident]
        assert v["vgpr_count"] <= 512 and v["vgpr_spill_count"] <= 8, (ident, v)
        if not big:
            continue
        blocks = re.split(r"\n\.LBB\d+_\d+:", bodies[ident])
        hot = [b for b in blocks if len(re.findall(r"\bv_mfma", b)) >= 60]
        assert len(hot) >= 4, (ident, len(hot))
        for b in hot:
            assert not re.findall(r"scratch_store", b), ident
            assert len(re.findall(r"scratch_load", b)) <= 1, ident


def test_ident_slots_issue_fewer_mfmas_in_the_designs_ratio():
    bodies = _bodies(chk.compile_isa(SRC))
    for ident, plain, big in _twins(bodies):
        ci, cp = _mfma_per_block(bodies[ident]), _mfma_per_block(bodies[plain])
        # the recurrent slot's body is the block that holds the most MFMAs (64-row tiles: 8 units x 2 halves; 16-row tiles: 2 units x 2 halves); the dual
        # kernel holds one per branch
        top_p = max(cp)
        slots_p = sorted(c for c in cp if c > top_p // 2)
        slots_i = sorted(c for c in ci if c > top_p // 2)
        assert slots_p and len(slots_p) == len(slots_i), (ident, slots_i, slots_p)   # found one to one
        for a, b in zip(slots_i, slots_p):
            assert a < b, (ident, a, b)
            assert b - a == (64 if big else 16), (ident, a, b)   # 16 MFMAs per m-tile of layer 0
        if big:
            assert abs(slots_i[0] / slots_p[0] - 960.0 / 1024.0) < 0.01, (ident, slots_i, slots_p)
