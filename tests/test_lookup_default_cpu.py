"""include/bzh2.h names the device as the place where every new key permutes its lookup columns (no device needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_names_the_device_as_the_default_lookup_permutation():
    hdr = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    text = hdr[hdr.index("/* Where bzh_prove_batch permutes the lookup"):hdr.index("} bzh_lookup_where;")]
    text = " ".join(text.replace("*", " ").split())
    assert re.search(r"BZH_LOOKUP_DEVICE \(every new key's default\)", text)
    assert not re.search(r"BZH_LOOKUP_HOST \(every new key's default\)", text)
