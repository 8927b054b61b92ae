"""tools/kernel_isa_diff.py gates every change to code shared by the chain kernels, so its parsing is held to
short synthetic listings in the layout hipcc writes: a kernel body between its label and .Lfunc_end, the descriptor numbers in
the .amdgpu_metadata block.  Same / reordered / DIFFERENT, label renumbering, and a loud failure where a field does not parse."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_isa_diff", os.path.join(ROOT, "tools", "kernel_isa_diff.py"))
K = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(K)

BODY = ["s_load_dword s2, s[0:1], 0x0", "v_mov_b32_e32 v1, 0", "s_waitcnt lgkmcnt(0)", "s_cmp_lt_i32 s2, 1", "s_cbranch_scc1 .LBB{n}_2",
        "v_add_u32_e32 v1, s2, v0", ".LBB{n}_2:", "global_store_dword v0, v1, s[4:5]", "s_endpgm"]
DESC = dict(agpr_count=0, group_segment_fixed_size=512, private_segment_fixed_size=0, sgpr_count=12, vgpr_count=4, vgpr_spill_count=0)


def listing(kernels, label_no=0, drop_field=None):
    """kernels: [(name, body lines, descriptor dict)] -> text of a device listing"""
    out = ["\t.text", "\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\""]
    for i, (name, body, _) in enumerate(kernels):
        out += ["\t.globl\t%s" % name, "\t.p2align\t8", "\t.type\t%s,@function" % name, "%s:    ; @%s" % (name, name), "; %bb.0:"]
        out += [ln.format(n=label_no + i) if ln.endswith(":") else "\t" + ln.format(n=label_no + i) + "    ; a comment" for ln in body]
        out += [".Lfunc_end%d:" % (label_no + i), "\t.size\t%s, .Lfunc_end%d-%s" % (name, label_no + i, name), "; -- End function",
                "\t.section\t.AMDGPU.csdata", "; NumVgprs: 4"]
    out += ["\t.amdgpu_metadata", "---", "amdhsa.kernels:"]
    for name, _, d in kernels:
        rows = [(".agpr_count", d["agpr_count"]), (".args", None), (".group_segment_fixed_size", d["group_segment_fixed_size"]),
                (".kernarg_segment_size", 12), (".name", name), (".private_segment_fixed_size", d["private_segment_fixed_size"]),
                (".sgpr_count", d["sgpr_count"]), (".sgpr_spill_count", 0), (".symbol", name + ".kd"), (".vgpr_count", d["vgpr_count"]),
                (".vgpr_spill_count", d["vgpr_spill_count"]), (".wavefront_size", 64)]
        first = True
        for key, val in rows:
            if key[1:] == drop_field:
                continue
            lead = "  - " if first else "    "
            first = False
            if key == ".args":
                out += [lead + ".args:", "      - .address_space:  global", "        .offset:         0", "        .size:           8"]
            else:
                out.append("%s%s: %s" % (lead, key, val))
    out += ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "...", "\t.end_amdgpu_metadata"]
    return "\n".join(out) + "\n"


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_same_reordered_different(tmp_path, capsys):
    swapped = [BODY[1], BODY[0]] + BODY[2:]                                   # two independent instructions the other way round
    longer = BODY[:5] + ["s_nop 0"] + BODY[5:]
    before = listing([("_Z1av", BODY, DESC), ("_Z1bv", BODY, DESC), ("_Z1cv", BODY, DESC), ("_Z1dv", BODY, DESC), ("_Z1ev", BODY, DESC)])
    after = listing([("_Z1av", BODY, DESC), ("_Z1bv", swapped, DESC), ("_Z1cv", longer, DESC), ("_Z1dv", swapped, dict(DESC, vgpr_count=5)),
                     ("_Z1ev", BODY, dict(DESC, private_segment_fixed_size=8))], label_no=40)      # other label numbers: ignored
    a, b = _write(tmp_path, "a.s", before), _write(tmp_path, "b.s", after)
    old, new = K.parse(a), K.parse(b)
    assert old["_Z1av"][1] == DESC and len(old["_Z1av"][0]) == len(BODY)      # comments, directives and blank lines are no instructions
    got = {k: K.classify(old[k], new[k])[0] for k in old}
    assert got == {"_Z1av": "same", "_Z1bv": "reordered", "_Z1cv": "DIFFERENT", "_Z1dv": "DIFFERENT", "_Z1ev": "DIFFERENT"}
    assert "s_nop+1" in K.classify(old["_Z1cv"], new["_Z1cv"])[1]
    assert "vgpr_count 4->5" in K.classify(old["_Z1dv"], new["_Z1dv"])[1]
    assert K.main([a, b]) == 1
    assert "kernels: 5  same: 1  reordered: 1  DIFFERENT: 3" in capsys.readouterr().out
    assert K.main([a, a]) == 0
    assert K.main([a, b, "--filter", "_Z1[ab]v"]) == 0                        # reordered alone does not fail the run


def test_lower_descriptor_is_reordered_and_a_missing_kernel_is_different(tmp_path, capsys):
    before = listing([("_Z1av", BODY, DESC), ("_Z1bv", BODY, DESC)])
    after = listing([("_Z1av", BODY, dict(DESC, vgpr_count=3))])
    a, b = _write(tmp_path, "a.s", before), _write(tmp_path, "b.s", after)
    assert K.classify(K.parse(a)["_Z1av"], K.parse(b)["_Z1av"])[0] == "reordered"
    assert K.main([a, b]) == 1
    assert "only in BEFORE" in capsys.readouterr().out


@pytest.mark.parametrize("field", K.FIELDS)
def test_a_descriptor_field_that_does_not_parse_is_an_error(tmp_path, field):
    p = _write(tmp_path, "a.s", listing([("_Z1av", BODY, DESC)], drop_field=field))
    with pytest.raises(ValueError, match=field):
        K.parse(p)


def test_a_kernel_without_a_body_or_a_listing_without_metadata_is_an_error(tmp_path):
    text = listing([("_Z1av", BODY, DESC)])
    with pytest.raises(ValueError, match="no instructions"):
        K.parse(_write(tmp_path, "a.s", text.replace("_Z1av:    ;", "_Z1av_renamed:    ;")))
    with pytest.raises(ValueError, match="no kernel"):
        K.parse(_write(tmp_path, "b.s", text.split("\t.amdgpu_metadata")[0]))
