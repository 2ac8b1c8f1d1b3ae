"""Writes tests/golden/sky_split_parent_v1.json: sha256 digests of the throughput lists (psoap_dag_plan_sky, psoap_dag_plan)
of tests/sky_split_cases.py as the planner built them BEFORE the skyline-aware split and order rules.  Run once against the
library of the commit in front of those rules (PSOAP_GP_LIB=<that libpsoap_gp.so>); tests/test_sky_split.py holds the list
under PSOAP_SKY_SPLIT=0, and every dense list, to these digests.

    PSOAP_GP_LIB=/path/to/parent/libpsoap_gp.so python tests/golden/make_sky_split_parent.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sky_split_cases          # noqa: E402

if __name__ == "__main__":
    with open(os.path.join(HERE, "sky_split_parent_v1.json"), "w") as f:
        d = sky_split_cases.parent_digests()
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(d[k], sort_keys=True)) for k in sorted(d)) + "\n}\n")
