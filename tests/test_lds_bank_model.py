"""scripts/lds_bank_model.py: every LDS access pattern of attn_bwd1b_kernel's query-tile loop costs
its ideal LDS-array cycle count under the MI355X lane-group / bank model (no GPU needed). The
offset functions are mirrored by hand from csrc/kernels/attention.hip; the last test evaluates the
kernel's own expressions against the mirrors, so a layout change in the kernel has to come through
the model."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("lds_bank_model", os.path.join(ROOT, "scripts", "lds_bank_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_loop_accesses_cost_their_ideal_cycles(model):
    pats = model.loop_patterns()
    # per wave and tile: 16 + 16 b128, 32 + 48 transposed reads, 8 b64 writes
    assert len(pats) == 8 * (16 + 16 + 32 + 8 + 48)
    for stage, instr, addr in pats:
        c, ideal = model.cycles(instr, addr)
        assert c == ideal, (stage, instr, [addr(l) for l in range(64)])


def test_model_reproduces_the_measured_conflicts_of_the_old_layouts(model):
    """With aoff for the K block and dst_off for dS^T, the dQ stage's transposed reads were 2-way
    conflicted: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 23.2 % measured at S = 512
    (profiles/attn_bwd_pmc_r6.txt)."""
    tab = model.summarize(model.loop_patterns(old=True))
    assert tab["dQ K^T tr"][1] == 2 * tab["dQ K^T tr"][2]
    assert tab["dQ dS^T tr"][1] == 2 * tab["dQ dS^T tr"][2]
    assert all(c == i for stage, (_, c, i) in tab.items() if not stage.startswith("dQ"))
    assert abs(model.conflict_share(8, old=True) - 0.232) < 0.002


def test_offset_functions_match_the_kernel_source(model):
    """The bodies of k1b_off / dst1b_off in attention.hip (integer expressions that read the same in
    Python) are evaluated here and compared with the model's mirrors, value by value."""
    src = open(os.path.join(ROOT, "csrc", "kernels", "attention.hip")).read()

    def kernel_fn(name):
        m = re.search(r"__device__ __forceinline__ int " + name + r"\(int (\w+), int (\w+)\) \{(.*?)\n\}", src, re.S)
        assert m, name
        a0, a1, body = m.groups()
        stmts = [st.strip() for st in " ".join(body.split()).split(";") if st.strip()]
        assert stmts[-1].startswith("return "), stmts

        def f(x, y):
            env = {a0: x, a1: y}
            for st in stmts[:-1]:
                var, expr = re.fullmatch(r"const int (\w+) = (.*)", st).groups()
                env[var] = eval(expr, {"__builtins__": {}}, env)
            return eval(stmts[-1][len("return "):], {"__builtins__": {}}, env)
        return f

    k_src, d_src = kernel_fn("k1b_off"), kernel_fn("dst1b_off")
    for row in range(256):
        for col in range(0, 64, 4):
            assert model.k1b_off(row, col) == k_src(row, col), (row, col)
            assert model.dst1b_off(row, col) == d_src(row, col), (row, col)
