"""The CPU fallbacks of the update kernels (sgd_update, adam_update, lamb_moments / lamb_norms /
lamb_apply, adamw_update) give bit for bit the outputs recorded from the commit named in
tests/golden/optimizer_kernels_sha256.json, section "cpu". Cases and inputs: optimizer_bits.py.

The section is regenerated with `python tests/test_optimizer_bits_cpu.py OUT.json [commit id]` on
the commit whose outputs are to be pinned."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import optimizer_bits as OB  # noqa: E402


@pytest.mark.parametrize("name", list(OB.CASES))
def test_cpu_fallback_bitwise_equal_to_recorded_parent(name):
    gold = OB.golden("cpu")
    sha = OB.run(name, "cpu")
    print(name, sha)
    assert sha == gold["cases"][name], f"outputs differ from those of commit {gold['commit']}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    OB.record("cpu", "cpu", sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "unknown")
