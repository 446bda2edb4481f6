"""Structure of pings_amd/csrc, read as text: where hipcub may be included and how many scratch carvers there are."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parents[1] / "pings_amd" / "csrc"
# devprim.hip serves every unit outside the 3D rasteriser; the rasteriser's own scan and sort fallbacks stay with it
HIPCUB_UNITS = {"devprim.hip", "raster_layout.hip", "raster_fwd.hip", "raster_bwd.hip", "raster_scan.hip", "tile_sort.hip"}


def _sources():
    files = sorted(p for p in CSRC.iterdir() if p.suffix in (".hip", ".hpp"))
    assert len(files) > 40
    return {p.name: p.read_text() for p in files}


def test_hipcub_is_included_by_devprim_and_the_rasteriser_only():
    including = {name for name, text in _sources().items() if re.search(r"#\s*include\s*[<\"]hipcub/", text)}
    assert "devprim.hip" in including
    assert including <= HIPCUB_UNITS, sorted(including - HIPCUB_UNITS)     # devprim.hpp among those that do not


def test_there_is_one_scratch_carver():
    found = [name for name, text in _sources().items() for _ in re.finditer(r"\bstruct\s+Carver\b", text)]
    assert found == ["common.hpp"]
