"""The HyP loss threshold out of the user's copy of the reference's ``models/DSPH/loss/codetable.xlsx``.

The reference reads it with xlrd at model construction (models/DSPH/DSPH.py:33-35):
``sheet_by_index(0).row(outputDim)[math.ceil(math.log(numclass, 2))].value``.  An .xlsx is a zip of XML parts, so the one cell is
read here with zipfile + xml.etree (no new dependency).  Rows and columns are 0-based as in xlrd: cell ``B2`` is (1, 1).  The table
itself is not shipped with this package."""
from __future__ import annotations

import math
import posixpath
import re
import zipfile
import xml.etree.ElementTree as ET

_NS = {"m": "http://schemas.openxmlformats.org/spreadsheetml/2006/main"}
_REL_ID = "{http://schemas.openxmlformats.org/officeDocument/2006/relationships}id"
_PKG_REL = "{http://schemas.openxmlformats.org/package/2006/relationships}Relationship"


def _first_sheet_part(z: zipfile.ZipFile) -> str:
    """path inside the archive of the workbook's first sheet (xlrd's sheet_by_index(0))"""
    try:
        book = ET.fromstring(z.read("xl/workbook.xml"))
        rid = book.find("m:sheets/m:sheet", _NS).get(_REL_ID)
        rels = ET.fromstring(z.read("xl/_rels/workbook.xml.rels"))
        target = next(r.get("Target") for r in rels.iter(_PKG_REL) if r.get("Id") == rid)
    except (KeyError, AttributeError, StopIteration):
        return "xl/worksheets/sheet1.xml"
    return target.lstrip("/") if target.startswith("/") else posixpath.normpath(posixpath.join("xl", target))


def _cell_ref(ref: str):
    m = re.fullmatch(r"([A-Z]+)(\d+)", ref)
    col = 0
    for ch in m.group(1):
        col = col * 26 + (ord(ch) - 64)
    return int(m.group(2)) - 1, col - 1


def read_cell(path: str, row: int, col: int):
    """value of the first sheet's cell (row, col), 0-based: a float for a number, a str for text, None when the cell is empty"""
    with zipfile.ZipFile(path) as z:
        sheet = ET.fromstring(z.read(_first_sheet_part(z)))
        shared = None
        for c in sheet.iterfind("m:sheetData/m:row/m:c", _NS):
            if _cell_ref(c.get("r")) != (row, col):
                continue
            kind = c.get("t", "n")
            if kind == "inlineStr":
                return "".join(t.text or "" for t in c.iter("{%s}t" % _NS["m"]))
            v = c.find("m:v", _NS)
            if v is None or v.text is None:
                return None
            if kind == "s":
                if shared is None:
                    shared = ["".join(t.text or "" for t in si.iter("{%s}t" % _NS["m"]))
                              for si in ET.fromstring(z.read("xl/sharedStrings.xml")).iterfind("m:si", _NS)]
                return shared[int(v.text)]
            if kind in ("str", "e"):
                return v.text
            if kind == "b":
                return float(int(v.text))
            return float(v.text)
    return None


def hyp_threshold(path: str, output_dim: int, numclass: int) -> float:
    """the threshold DSPH's HyP loss uses for `output_dim` bits and `numclass` classes (models/DSPH/DSPH.py:33-35)"""
    col = math.ceil(math.log(numclass, 2))                 # the reference's expression, kept as it is
    value = read_cell(path, output_dim, col)
    if not isinstance(value, float):
        raise ValueError("codetable %s: cell (row %d, column %d) for %d bits / %d classes holds no number (%r)"
                         % (path, output_dim, col, output_dim, numclass, value))
    return value
