"""tools/kernel_disasm.py --by-body: the matching step alone, on hand-written instruction lists (no compiler, no GPU)."""
import importlib.util
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_disasm", ROOT / "tools" / "kernel_disasm.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BODY = ["\ts_load_dwordx2 s[0:1], s[4:5], 0x0", "\tv_lshlrev_b32_e32 v1, 2, v0", "\ts_waitcnt lgkmcnt(0)",
        "\tglobal_load_dword v2, v1, s[0:1]", "\ts_waitcnt vmcnt(0)", "\tv_add_f32_e32 v2, v2, v2",
        "\tglobal_store_dword v1, v2, s[0:1]", "\ts_endpgm"]


def test_match_bodies_across_a_rename():
    kd = _tool()
    renamed = [line.replace("v2", "v7").replace("v1", "v3") for line in BODY]  # the same code in other registers
    other = BODY[:5] + ["\tv_mul_f32_e32 v2, v2, v2"] + BODY[6:]               # another opcode in the same place
    shorter = BODY[:2] + BODY[3:]                                              # one instruction fewer
    assert renamed != BODY and kd.opcodes(renamed) == kd.opcodes(BODY)
    assert kd.opcodes(BODY)[:3] == ["s_load_dwordx2", "v_lshlrev_b32_e32", "s_waitcnt"]

    old = {"kept": BODY, "plain_kernel": BODY + ["\ts_nop 0"], "w_kernel": other, "q_kernel": BODY + ["\ts_nop 1"],
           "changed": BODY, "gone": shorter + ["\ts_nop 2"]}
    new = {"kept": BODY,                                      # same symbol, same body
           "kernel<false>": BODY + ["\ts_nop 0"],             # renamed symbol, same body
           "kernel<true>": other,                             # renamed symbol, same body (another one)
           "kernel<quant>": renamed + ["\ts_nop 1"],          # renamed symbol, same opcodes, other registers
           "changed": other + ["\ts_nop 3"],                  # same symbol, another opcode sequence
           "added": ["\ts_endpgm"]}
    got = kd.match_bodies(old, new)
    assert got == {"kept": ("identical", "kept"), "plain_kernel": ("identical", "kernel<false>"),
                   "w_kernel": ("identical", "kernel<true>"), "q_kernel": ("renamed-registers", "kernel<quant>"),
                   "changed": ("different", "changed"), "gone": ("missing", None)}
    # a symbol of NEW answers for one symbol of OLD only, and an identical body wins over a merely similar one
    twice = kd.match_bodies({"a": BODY, "b": BODY}, {"c": BODY, "d": renamed})
    assert twice == {"a": ("identical", "c"), "b": ("renamed-registers", "d")}
    assert kd.match_bodies({"a": BODY}, {"d": renamed, "c": BODY}) == {"a": ("identical", "c")}
    assert kd.match_bodies({"a": BODY}, {}) == {"a": ("missing", None)}
