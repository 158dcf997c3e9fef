"""``python -m pymasc_amd``: the ``pymasc`` command (pymasc_amd.cli)."""
import sys

from pymasc_amd import cli

sys.exit(cli.main())
