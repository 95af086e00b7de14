"""Child process of tests/test_gpu_entropy_paths.py's test of KVZ_HIP_ENTROPY_LANES: the library reads the variable once per process, so each value gets a fresh one.
One small intra group and one stage picture through the device's coder; exit status 0 when both equal the oracle.  usage: entropy_lanes_child.py (the variable in the
environment)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import entropy_atlas as ea  # noqa: E402
import entropy_common as ec  # noqa: E402
import flatapi  # noqa: E402


def main():
    import kvazaar_amd
    oracle, lib = flatapi.load_oracle(), kvazaar_amd.load_library()
    name, w, h, sw, pictures = ea.stage_groups()[0]
    for group in (ea.intra_groups()[1], (name, w, h, sw, pictures[1:2])):
        if ec.device_intra_group(lib, group) != ec.atlas_oracle_group(oracle, group):
            print(f"lanes {os.environ.get('KVZ_HIP_ENTROPY_LANES')}: {group[0]} differs from the oracle")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
