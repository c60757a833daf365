"""tools/listing_diff.py: what it keeps of a listing.  The comparison is between instruction streams, so comment lines,
directives and the per-compilation __hip_cuid_* symbol must drop out, labels and instructions must stay, and a kernel's
figures must come from its own metadata block.  No compiler, no GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LISTING = """\
\t.text
\t.globl\t_Z3fooPf
\t.p2align\t8
\t.type\t_Z3fooPf,@function
_Z3fooPf:                               ; @_Z3fooPf
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0     ; a trailing comment
\tv_mov_b32_e32 v0, {imm}
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
\ts_cbranch_scc1 .LBB0_1
\ts_endpgm
\t.section\t.rodata,"a",@progbits
.Lfunc_end0:
\t.size\t_Z3fooPf, .Lfunc_end0-_Z3fooPf
; NumVgprs: 1
_Z3barv:
\ts_endpgm
.Lfunc_end1:
\t.type\t__hip_cuid_{cuid},@object
__hip_cuid_{cuid}:
\t.byte\t0
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .group_segment_fixed_size: {lds}
    .name:           _Z3fooPf
    .private_segment_fixed_size: 0
    .sgpr_count:     10
    .sgpr_spill_count: 0
    .symbol:         _Z3fooPf.kd
    .vgpr_count:     1
    .vgpr_spill_count: 0
  - .agpr_count:     0
    .group_segment_fixed_size: 64
    .name:           _Z3barv
    .private_segment_fixed_size: 16
    .sgpr_count:     4
    .sgpr_spill_count: 0
    .symbol:         _Z3barv.kd
    .vgpr_count:     3
    .vgpr_spill_count: 2
amdhsa.version:
  - 1
  - 2
...
\t.end_amdgpu_metadata
"""


def _tool():
    spec = importlib.util.spec_from_file_location("listing_diff", os.path.join(ROOT, "tools", "listing_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parse_keeps_instructions_and_labels_only():
    funcs, figures = _tool().parse(LISTING.format(imm="0", cuid="aaaa", lds=128).split("\n"))
    assert list(funcs) == ["_Z3fooPf", "_Z3barv"]          # neither the cuid symbol nor a metadata key is a function
    assert funcs["_Z3fooPf"] == ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mov_b32_e32 v0, 0", ".LBB0_1:",
                                 "s_cbranch_scc1 .LBB0_1", "s_endpgm"]
    assert funcs["_Z3barv"] == ["s_endpgm"]
    assert figures["_Z3fooPf"] == {"vgpr_count": 1, "sgpr_count": 10, "vgpr_spill_count": 0, "sgpr_spill_count": 0,
                                   "private_segment_fixed_size": 0, "group_segment_fixed_size": 128}
    assert figures["_Z3barv"]["group_segment_fixed_size"] == 64 and figures["_Z3barv"]["vgpr_spill_count"] == 2
    assert figures["_Z3barv"]["private_segment_fixed_size"] == 16


def test_cuid_and_figures_do_not_decide_equality_an_instruction_does():
    parse = _tool().parse
    base, _ = parse(LISTING.format(imm="0", cuid="aaaa", lds=128).split("\n"))
    other_cuid, fig = parse(LISTING.format(imm="0", cuid="bbbb", lds=256).split("\n"))
    assert other_cuid == base and fig["_Z3fooPf"]["group_segment_fixed_size"] == 256
    changed, _ = parse(LISTING.format(imm="1", cuid="aaaa", lds=128).split("\n"))
    assert changed["_Z3fooPf"] != base["_Z3fooPf"] and changed["_Z3barv"] == base["_Z3barv"]
