"""The HIP update kernels (sgd_kernel, adam_kernel, lamb_moments / lamb_norms / lamb_apply,
adamw_kernel) give bit for bit the outputs recorded on an MI355X from the commit named in
tests/golden/optimizer_kernels_sha256.json, section "gpu": the kernels' source may be reshaped,
their arithmetic may not. Cases and inputs: optimizer_bits.py.

The section is regenerated with `python tests/test_optimizer_bits_gpu.py OUT.json [commit id]` on
a build of the commit whose outputs are to be pinned."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import optimizer_bits as OB  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(OB.CASES))
def test_kernels_bitwise_equal_to_recorded_parent(name):
    gold = OB.golden("gpu")
    sha = OB.run(name, "cuda")
    print(name, sha)
    assert sha == gold["cases"][name], f"outputs differ from those of commit {gold['commit']}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    OB.record("gpu", "cuda", sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "unknown")
