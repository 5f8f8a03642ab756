"""scripts/gemm_isa_diff.py: the normaliser and the per-kernel verdict on
short synthetic assembly. What must not count as a difference (a renamed
block label, a renamed mangled symbol, another __hip_cuid_ hash, comments,
directives) and what must (two instructions swapped, another register
number, another resource figure). CPU only; hipcc is not invoked."""

import importlib.util
import sys
from pathlib import Path

_spec = importlib.util.spec_from_file_location(
    "gemm_isa_diff",
    Path(__file__).resolve().parent.parent / "scripts" / "gemm_isa_diff.py")
isa = importlib.util.module_from_spec(_spec)
sys.modules[_spec.name] = isa  # the script's dataclass looks its module up
_spec.loader.exec_module(isa)


def asm(body, name="_ZN3hpk12_GLOBAL__N_16k_gemmILb0ELb1EEEvPfi", vgprs=90,
        cuid="10913585024dbe29", end=0):
    return f"""\t.text
\t.globl\t{name} ; -- Begin function {name}
\t.p2align\t8
\t.type\t{name},@function
{name}: ; @{name}
; %bb.0:
{body}
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr 90
\t.end_amdhsa_kernel
.Lfunc_end{end}:
\t.size\t{name}, .Lfunc_end{end}-{name}
; codeLenInByte = 3044
; NumVgprs: {vgprs}
; NumAgprs: 0
; ScratchSize: 0
; LDSByteSize: 65536 bytes/workgroup (compile time only)
; Occupancy: 4
\t.type\t__hip_cuid_{cuid},@object ; @__hip_cuid_{cuid}
\t.globl\t__hip_cuid_{cuid}
__hip_cuid_{cuid}:
"""


BODY = """\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_lshlrev_b32_e32 v1, 4, v0
.LBB0_1: ; =>This Inner Loop Header: Depth=1
\ts_waitcnt vmcnt(2)
\tv_mfma_f32_16x16x32_bf16 v[2:5], v[6:9], v[10:13], v[2:5]
\ts_cbranch_scc1 .LBB0_1
\tglobal_store_dword v1, v2, s[0:1]"""


def verdicts(a, b):
    return [(v, ka and ka.instructions, kb and kb.instructions)
            for _, ka, kb, v in isa.compare(a, b)]


def test_normalise_keeps_instructions_and_drops_the_rest():
    stream = isa.normalise(BODY + "\n\t.p2align 6\n\n ; a comment\n")
    assert stream == [
        "s_load_dwordx2 s[0:1], s[4:5], 0x0",
        "v_lshlrev_b32_e32 v1, 4, v0",
        "L0:",
        "s_waitcnt vmcnt(2)",
        "v_mfma_f32_16x16x32_bf16 v[2:5], v[6:9], v[10:13], v[2:5]",
        "s_cbranch_scc1 L0",
        "global_store_dword v1, v2, s[0:1]",
    ]


def test_split_kernels_reads_name_stream_and_resources():
    ks = isa.split_kernels(asm(BODY))
    (name, k), = ks.items()
    assert name == "_ZN3hpk12_GLOBAL__N_16k_gemmILb0ELb1EEEvPfi"
    assert k.instructions == 7  # BODY's 6 + s_endpgm; the label is not one
    assert k.resources == {"NumVgprs": 90, "NumAgprs": 0, "ScratchSize": 0,
                           "LDSByteSize": 65536, "Occupancy": 4}


def test_same_text_is_identical():
    assert verdicts(asm(BODY), asm(BODY)) == [("identical", 7, 7)]


def test_renamed_label_is_identical():
    other = BODY.replace(".LBB0_1", ".LBB3_7")
    assert other != BODY
    assert verdicts(asm(BODY), asm(other, end=3)) == [("identical", 7, 7)]


def test_changed_cuid_hash_is_identical():
    assert verdicts(asm(BODY), asm(BODY, cuid="f00dfeed01234567")) == [
        ("identical", 7, 7)]


def test_symbol_reference_renamed_with_its_symbol_is_identical():
    ref = "\ts_getpc_b64 s[2:3]\n\ts_add_u32 s2, s2, {0}@rel32@lo+4\n" + BODY
    a = asm(ref.format("_ZN3hpk3tabE"))
    b = asm(ref.format("_ZN3hpk5tableE"))
    assert verdicts(a, b) == [("identical", 9, 9)]


def test_reordered_pair_of_instructions_is_different():
    lines = BODY.splitlines()
    lines[0], lines[1] = lines[1], lines[0]
    assert verdicts(asm(BODY), asm("\n".join(lines))) == [("different", 7, 7)]


def test_changed_register_number_is_different():
    other = BODY.replace("v[10:13]", "v[14:17]")
    assert other != BODY
    assert verdicts(asm(BODY), asm(other)) == [("different", 7, 7)]


def test_changed_wait_count_is_different():
    other = BODY.replace("vmcnt(2)", "vmcnt(0)")
    assert verdicts(asm(BODY), asm(other)) == [("different", 7, 7)]


def test_same_stream_other_register_count_is_different():
    assert verdicts(asm(BODY), asm(BODY, vgprs=92)) == [("different", 7, 7)]


def test_added_and_removed_kernels_are_reported():
    two = asm(BODY) + asm(BODY, name="_ZN3hpk5otherEv", end=1)
    assert verdicts(asm(BODY), two) == [("identical", 7, 7),
                                        ("added", None, 7)]
    assert verdicts(two, asm(BODY)) == [("identical", 7, 7),
                                        ("removed", 7, None)]
