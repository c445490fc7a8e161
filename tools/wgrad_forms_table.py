#!/usr/bin/env python3
"""Print the weight-gradient form table of DESIGN.md (section 8.3) from the test table, tests/wgrad_cases.py.

    python tools/wgrad_forms_table.py

tests/test_wgrad_forms.py fails when DESIGN.md no longer holds what this prints."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import wgrad_cases  # noqa: E402

if __name__ == "__main__":
    print(wgrad_cases.design_table())
