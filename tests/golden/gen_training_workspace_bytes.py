"""Records tests/golden/training_workspace_bytes.json: the workspace sizes of the three training entry points over the grid of
tests/test_training_api_cpu.py, from the library as built.  Run it only when a workspace layout is meant to change."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.test_training_api_cpu import GOLDEN, workspace_table  # noqa: E402

json.dump(workspace_table(), open(GOLDEN, "w"), indent=0, sort_keys=True)
