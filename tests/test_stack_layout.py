"""The buffer plans of a stack (semantichuman_amd/stack.py): every arena offset, mask, size and shape of the fp32 and the bf16 path,
compared exactly with tests/golden/stack_plans.json.  The plan reads the steps' shapes only, so the stacks are built and "uploaded"
on the CPU (as in tests/test_stack_plan.py).

The golden file was recorded from the two hand-written plans (`_plan`, offsets in floats, and `_plan_bf16`, in bytes) that the one
layout routine replaced; `flatten` takes those dicts as well as the plan type and brings everything to bytes.  A change of a
workspace size or of a form rule moves offsets: re-record with `python tests/test_stack_layout.py --record` and show the diff."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from semantichuman_amd import _lib                                      # noqa: E402
from tests.test_stack_plan import _model_stacks, _sweep_stacks         # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "stack_plans.json")
F32_BATCHES = (16, 48, 64, 512)
BF16_CASES = [(B, out_is_f32) for B in (16, 64) for out_is_f32 in (False, True)]
# the hand-written fp32 plan kept these in floats; everything else it held was bytes already
_F32_IN_FLOATS = ("f_total", "b_total", "p_total", "dpre_last_off")
_P3_FIELDS = ("pl_off", "pl_mask", "pl_total", "in_img", "gpl_off", "gpl_mask", "dpl_off", "dpl_mask", "gpl_total", "wf3_off", "wf3_mask",
              "wf3t_off", "wf3t_mask", "wf3_jobs", "wf3_total")
_FIELDS = ("out_rows", "out_ch", "npar", "shapes", "f_off", "f_total", "dpre_last_off", "g_off", "g_mask", "wt_off", "wt_mask", "ws_off",
           "ws_mask", "ws_bytes", "b_total", "dW_off", "db_off", "p_total")


def _ints(v):
    if v is None:
        return [0, 0]                                                   # a parameter index no conv step uses has no shape
    if isinstance(v, (list, tuple)):
        return [x for e in v for x in _ints(e)]
    return [int(x) for x in np.asarray(v).reshape(-1)]


def flatten(plan, bf16):
    """name -> list of integers, offsets and totals in bytes."""
    if isinstance(plan, dict):                                          # the plans before the one layout routine
        d = {k: plan[k] for k in _FIELDS if k in plan}
        d.setdefault("dpre_last_off", 0)
        if bf16:
            d["p_total"] = 4 * plan["p_total"]
            d.update(wf_off=plan["wf_off"], wf_mask=plan["wf_mask"])
        else:
            d.update({k: 4 * plan[k] for k in _F32_IN_FLOATS})
            d.update({k: plan[k] for k in _P3_FIELDS})
    else:                                                               # one mask for all that a conv step alone has
        d = {k: plan.conv_mask if k in ("wt_mask", "ws_mask") else getattr(plan, k) for k in _FIELDS}
        if bf16:
            d.update(wf_off=plan.wf_off, wf_mask=plan.conv_mask)
        else:
            d.update({k: getattr(plan, k) for k in _P3_FIELDS})
    return {k: _ints(v) for k, v in d.items()}


def _plan_of(stack, B, c0, bf16, out_is_f32=True):
    if hasattr(stack, "_plan_bf16"):                                    # recording, at a commit that still has the two plans
        if not bf16:
            return stack._plan(B, c0)
        a, b = (stack._plan_bf16(B, c0, x_is_f32, out_is_f32) for x_is_f32 in (False, True))
        assert flatten(a, True) == flatten(b, True)                     # the input's type never moved an offset
        return a
    return stack._plan(B, c0, bf16=bf16, out_is_f32=out_is_f32)


def _stacks():
    out = {}
    for tpl in ("template6890.npz", "template27554.npz"):
        for name, (stack, c0, *_) in zip(("enc", "dec"), _model_stacks(tpl)):
            out["%s/%s" % (tpl.split(".")[0], name)] = (stack, c0)
    for k, (stack, c0, *_) in enumerate(_sweep_stacks()):
        out["sweep%02d" % k] = (stack, c0)
    return out


@pytest.fixture(scope="module")
def stacks():
    assert not [k for k in os.environ if k.startswith("SH_")], "the golden plans are those of the default switches"
    return _stacks()


def _all_plans(stacks):
    out = {}
    for name, (stack, c0) in stacks.items():
        for B in F32_BATCHES:
            out["%s/f32/B%d" % (name, B)] = flatten(_plan_of(stack, B, c0, False), False)
        for B, o32 in BF16_CASES:
            out["%s/bf16/B%d/%s" % (name, B, "out_f32" if o32 else "out_bf16")] = flatten(_plan_of(stack, B, c0, True, o32), True)
    return out


def test_offsets_match_the_recorded_plans(stacks):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _all_plans(stacks)
    assert sorted(got) == sorted(want)
    for name in want:
        assert sorted(got[name]) == sorted(want[name]), name
        for k in want[name]:
            assert got[name][k] == want[name][k], (name, k)


def test_every_offset_is_256_byte_aligned(stacks):
    for name, p in _all_plans(stacks).items():
        for k, v in p.items():
            if k.endswith("_off") or k.endswith("_total"):
                assert all(x % 256 == 0 for x in v), (name, k)
        assert all(x % 256 == 0 for x in p.get("wf3_jobs", [])[2::3]), name


def _disjoint(regions, total, what):
    """regions: (offset, bytes) of every live buffer of one arena - none overlaps the next, all inside the arena."""
    end = 0
    for off, size in sorted(regions):
        assert off >= end, (what, off, end)
        end = off + size
    assert end <= total, (what, end, total)


def _check_regions(stack, B, c0, bf16, out_is_f32):
    lib = _lib.load()
    p = _plan_of(stack, B, c0, bf16, out_is_f32)
    steps, n = stack.steps, len(stack.steps)
    esz, esz_last = (2, 4 if out_is_f32 else 2) if bf16 else (4, 4)
    conv = [i for i in range(n) if steps[i].kind == "conv"]
    # forward arena: one buffer per step but the last; a folded up-sampling appends to its predecessor's (the documented alias)
    fwd = []
    for i in range(n - 1):
        if stack._extends(i):
            assert p.f_off[i] == p.f_off[i - 1]
        else:
            fwd.append((int(p.f_off[i]), stack._buffer_rows(i) * B * p.out_ch[i] * esz))
    if bf16:
        fwd += [(int(p.wf_off[i]), int(lib.sh_conv_wfrag_bytes(steps[i].S, steps[i].cin, steps[i].cout))) for i in conv]
    _disjoint(fwd, p.f_total, "forward")
    # backward arena: dpre of the last step | the two alternating input-gradient regions, each shared by the steps of one parity |
    # per conv the backward-data operand and the partial slabs
    last, bwd = steps[-1], []
    if last.kind == "conv":
        bwd.append((p.dpre_last_off, (last.R + last.n_extra) * B * last.cout * esz_last))
    need = [0, 0]
    for i in range(1, n):
        st, prev = steps[i], steps[i - 1]
        rows = (st.n_in if st.kind == "conv" else st.csr.cols) + (prev.n_extra if prev.kind == "conv" else 0)
        need[i % 2] = max(need[i % 2], rows * B * p.out_ch[i - 1] * esz)
        assert p.g_mask[i] == 1 and p.g_off[i] == p.g_off[2 - i % 2]
    assert p.g_mask[0] == 0
    bwd += [(int(p.g_off[i]), need[i % 2]) for i in (1, 2) if i < n]
    for i in conv:
        st = steps[i]
        bwd.append((int(p.wt_off[i]), int(lib.sh_conv_wfrag_bytes(st.S, st.cout, st.cin)) if bf16 else st.cin * st.S * st.cout * 4))
        bwd.append((int(p.ws_off[i]), int(p.ws_bytes[i])))
    assert [int(m) for m in p.conv_mask] == [int(i in conv) for i in range(n)]
    _disjoint(bwd, p.b_total, "backward")
    flat = []
    for i in conv:
        st = steps[i]
        assert tuple(p.shapes[st.param]) == (st.cout, st.S * st.cin)
        flat += [(int(p.dW_off[st.param]), st.cout * st.S * st.cin * 4), (int(p.db_off[st.param]), st.cout * 4)]
    _disjoint(flat, p.p_total, "parameter gradients")
    if bf16:
        return
    # three-plane form: images of the forward buffers | images of the gradients | weight fragments
    q, img = p, []
    for i in range(n - 1):
        if stack._extends(i):
            assert (q.pl_off[i], q.pl_mask[i]) == (q.pl_off[i - 1], q.pl_mask[i - 1])
        elif q.pl_mask[i]:
            img.append((int(q.pl_off[i]), int(lib.sh_p3_bytes(stack._buffer_rows(i), B, p.out_ch[i]))))
    _disjoint(img, q.pl_total, "forward images")
    gimg = [(int(q.gpl_off[i]), int(lib.sh_p3_bytes(steps[i - 1].R + steps[i - 1].n_extra, B, steps[i - 1].cout)))
            for i in range(1, n) if q.gpl_mask[i]]
    if q.dpl_mask:
        gimg.append((int(q.dpl_off), int(lib.sh_p3_bytes(last.R + last.n_extra, B, last.cout))))
    _disjoint(gimg, q.gpl_total, "gradient images")
    frag = []
    for i, t, off in q.wf3_jobs:
        st = steps[i]
        assert off == (q.wf3t_off if t else q.wf3_off)[i] and (q.wf3t_mask if t else q.wf3_mask)[i] == 1
        frag.append((int(off), int(lib.sh_conv_wfrag3_bytes(st.S, st.cout if t else st.cin, st.cin if t else st.cout))))
    assert len(frag) == int(np.sum(q.wf3_mask) + np.sum(q.wf3t_mask))
    _disjoint(frag, q.wf3_total, "plane weight fragments")


def test_live_regions_do_not_overlap(stacks):
    for stack, c0 in stacks.values():
        for B in F32_BATCHES:
            _check_regions(stack, B, c0, False, True)
        for B, o32 in BF16_CASES:
            _check_regions(stack, B, c0, True, o32)


def test_both_paths_lay_out_the_parameter_gradients_alike(stacks):
    for name, (stack, c0) in stacks.items():
        for B, o32 in BF16_CASES:
            a, b = flatten(_plan_of(stack, B, c0, False), False), flatten(_plan_of(stack, B, c0, True, o32), True)
            for k in ("dW_off", "db_off", "p_total", "shapes", "npar", "out_rows", "out_ch"):
                assert a[k] == b[k], (name, B, k)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_stack_layout.py --record"
    assert not [k for k in os.environ if k.startswith("SH_")]
    with open(GOLDEN, "w") as f:
        json.dump(_all_plans(_stacks()), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("recorded %s: %d bytes" % (GOLDEN, os.path.getsize(GOLDEN)))
