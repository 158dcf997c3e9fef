"""Child of tests/test_cli.py: one rank of ``python -m pymasc_amd`` on the test context -- the gloo backend, every rank on the
one stand-in "GPU", ``cli.main`` under the RANK / WORLD_SIZE / MASTER_* that launch.spawn_ranks sets."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

from pymasc_amd import cli, ffi  # noqa: E402
from tests.fake_context import FakeContext  # noqa: E402


def main():
    os.environ["PMX_DIST_BACKEND"] = "gloo"
    torch.cuda.device_count = lambda: 1                 # the ranks share the one device, as on a one-GPU box
    ffi.Context = lambda device=0: FakeContext()
    return cli.main(sys.argv[1:])


if __name__ == "__main__":
    sys.exit(main())
