"""`conftest.bar` for the segmented-AdamW tests, with the recorded MI355X baselines in a file of these tests' own
(tests/golden/parity_bars_adamw_seg.json: the EGOM2P_RECORD_BARS values of the names below, one JSON object): a measurement is held to
the stated tolerance by `bar` and to its recorded value plus conftest.bar's 30 % margin here; a recording run checks the tolerance only."""
import json
import os

from conftest import GOLDEN_DIR, bar

_PATH = os.path.join(GOLDEN_DIR, "parity_bars_adamw_seg.json")
_BASE = json.load(open(_PATH)) if os.path.exists(_PATH) else {}


def held(name, value, hard, rel_margin=0.30):
    value = bar(name, value, hard=hard, rel_margin=rel_margin)
    if not os.environ.get("EGOM2P_RECORD_BARS"):
        assert name in _BASE, (name, "has no recorded baseline in parity_bars_adamw_seg.json")
        assert value <= _BASE[name] * (1.0 + rel_margin), (name, value, "recorded baseline", _BASE[name])
    return value
