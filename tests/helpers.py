"""Shared helpers for the test-suite (config loading, synthetic inputs of SURVEY.md section 8d live in the package)."""
import importlib
import os
import sys

from sampling_gpmpc_amd.workloads import PARAMS_DIR as PARAMS, closed_loop_params, fs_params, load_params, synthetic_u_ff  # noqa: F401

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
TOOLS = os.path.join(REPO, "tools")


def load_tool(name):
    """tools/<name>.py as a module: the same object for the same name within a process (tools/isa.py compiles a kernel file once
    per process), found the way a tool run as a script finds isa.py beside it."""
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    return importlib.import_module(name)
