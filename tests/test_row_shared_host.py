"""Row-shared windows (option "row_shared") as the form selection reports them without a GPU: sga_explain_route names
the form for the C2a query only when the option forces it -- the default leaves it to sga_autotune, which a query
cannot know about, so the golden route table's answers stay as they are."""
import json
import os


def _c2a_query():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_table.json")) as f:
        cases = json.load(f)["cases"]
    return next(c for c in cases if c["name"].startswith("BASELINE c2a"))


def test_explain_route_names_the_form_only_when_forced():
    from spin_glass_anneal_rl_amd import _native as N
    c = _c2a_query()
    assert N.explain_route(N.route_query(**c["query"])) == c["explain"]  # default 2: by autotune
    forced = N.explain_route(N.route_query(**{**c["query"], "options": {"row_shared": 1}}))
    assert forced.startswith(c["explain"].split(" cached=")[0]) and " sweep=row-shared(W=1024)" in forced
    assert "look_ahead=2" in forced
    assert N.explain_route(N.route_query(**{**c["query"], "options": {"row_shared": 0}})) == c["explain"]
    # problems the form does not serve: real-valued couplings (fp64 sums), no accept table, several models, look-ahead off
    for change in ({"acc": 1}, {"table_m": 0}, {"n_models": 2}, {"clf_ok": 0}, {"options": {"row_shared": 1, "look_ahead": 0}}):
        q = {**c["query"], "options": {"row_shared": 1}, **change}
        assert "row-shared" not in N.explain_route(N.route_query(**q)), change


def test_row_shared_options_exist_with_their_defaults():
    from spin_glass_anneal_rl_amd import _native as N
    names = N.option_names()
    assert "row_shared" in names and "row_shared_window" in names
    q = N.route_query()
    assert q.opt[names.index("row_shared")] == 2 and q.opt[names.index("row_shared_window")] == 0
