"""Regenerates tests/golden/f16_xml_tables.json: what the reference's aircraft/f16/f16.xml says
about each aerodynamic coefficient function, recorded as the file's own text (the numbers are
kept as the strings the XML holds, so the test parses them itself): the function's name and the
line it starts on, the property names of its product, and its constant or its table data.

    python tests/golden/make_f16_xml_tables.py <path to the reference's aircraft/f16/f16.xml>

tests/test_oracle_golden.py::test_fixture_matches_reference_xml holds f16_model.json (made by
tools/gen_tables.py) against this record."""
import json
import os
import sys
import xml.etree.ElementTree as ET

if __name__ == "__main__":
    path = sys.argv[1]
    with open(path) as f:
        lines = f.read().splitlines()
    aero = ET.parse(path).getroot().find("aerodynamics")
    fns = []
    for axis in aero.findall("axis"):
        for fn in axis.findall("function"):
            name = fn.get("name")
            prod = fn.find("product")
            ent = {"name": name,
                   "line": next(i + 1 for i, ln in enumerate(lines) if 'function name="%s"' % name in ln),
                   "props": [p.text for p in prod.findall("property")]}
            tab = prod.find("table")
            if tab is None:
                ent["value"] = prod.find("value").text
            else:
                ent["table_data"] = tab.find("tableData").text
            fns.append(ent)
    out = {"source": "aircraft/f16/f16.xml of the reference, <aerodynamics> (tests/golden/make_f16_xml_tables.py)",
           "functions": fns}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "f16_xml_tables.json"), "w") as f:
        json.dump(out, f, indent=1)
