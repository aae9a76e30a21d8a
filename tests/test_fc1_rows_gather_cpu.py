"""Host side of ``TUNING.fc1_rows_gather`` (engine_core.fc1_rows_gather_enabled): when the fc1 backward reads its gradient rows through
the row table and when it keeps the copy path - source of 2 GiB and more, no compact row space, switch off - and the workspace's
on-request buffers."""
import pytest

from scene_graph_commonsense_amd import engine_core as E


def _wm(objrows=100, prow=True, rowsrc=True):
    return dict(prow=object() if prow else None, rowsrc=object() if rowsrc else None, objrows=objrows)


def test_default_is_on_and_reads_the_environment(monkeypatch):
    assert E.Tuning().fc1_rows_gather
    monkeypatch.setenv("SGC_TUNING", "fc1_rows_gather=0")
    assert not E.Tuning.from_env().fc1_rows_gather


def test_gather_path_inside_the_range():
    assert E.FC1_GATHER_ROW_LIMIT * 4096 * 2 == 1 << 31
    assert E.fc1_rows_gather_enabled(_wm(), 512)
    # the benchmark's minibatch, 8 x 64 objects: 32 256 pairs + zero row + about 21 k per-object rows
    assert E.fc1_rows_gather_enabled(_wm(objrows=21000), 8 * 64 * 63)


@pytest.mark.parametrize("ppad,objrows,want", [(262144 - 1 - 100 - 1, 100, True), (262144 - 1 - 100, 100, False), (262144, 0, False),
                                               (64, 262144, False)])
def test_copy_path_from_the_limit_on(ppad, objrows, want):
    """Ppad + 1 + per-object rows < 262144 rows of 8 KiB: the last source row ends below 2 GiB."""
    assert E.fc1_rows_gather_enabled(_wm(objrows=objrows), ppad) == want


def test_copy_path_without_the_compact_row_space_or_the_table():
    assert not E.fc1_rows_gather_enabled(None, 512)
    assert not E.fc1_rows_gather_enabled(_wm(prow=False), 512)
    assert not E.fc1_rows_gather_enabled(_wm(rowsrc=False), 512)


def test_copy_path_with_the_switch_off():
    with E.tuning(fc1_rows_gather=False):
        assert not E.fc1_rows_gather_enabled(_wm(), 512)
    assert E.fc1_rows_gather_enabled(_wm(), 512)


def test_on_request_buffers_are_built_when_read_and_never_stored():
    b = E._Buffers()
    calls = []
    b["real"] = 1
    b.virtual["gwm"] = lambda: calls.append(1) or "built"
    assert "gwm" not in b and b.get("gwm") is None and list(b) == ["real"]
    assert b["gwm"] == "built" and b["gwm"] == "built" and len(calls) == 2 and "gwm" not in b
    with pytest.raises(KeyError):
        b["other"]
