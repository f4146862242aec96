"""The Python constant of IFE_OPT_Z_SWEEP is the header's (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_value_matches_the_header(ife):
    header = open(os.path.join(ROOT, "include", "ife_hip.h")).read()
    assert ife.OPT_Z_SWEEP == int(re.search(r"IFE_OPT_Z_SWEEP\s*=\s*(\d+)", header).group(1)) == 12
