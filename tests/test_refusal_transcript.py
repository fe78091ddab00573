"""The refusals of the C ABI's batched entry points, exactly: every call below is made with a NULL handle and fake pointers that
are never dereferenced, and the whole list of (return code, lf_mkd_last_error(NULL)) is held to tests/golden/refusal_transcript.json.
The api tests beside this one assert substrings; this one pins the order of every chain and every message, character by
character, so that the entry layer can be reorganised without any copy of a check drifting.

The JSON is a recording of the library as it was BEFORE the entry layer was split by subsystem.  It is made by running this
file as a script (`LF_MKD_LIB=<that library> python tests/test_refusal_transcript.py --record`) with a library built from that commit, and
is never regenerated from a later one: a difference is a changed contract, to be explained, not re-recorded."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "refusal_transcript.json")

P, ODD2, ODD4, ODD8 = 64, 66, 68, 72   # fake addresses: aligned to 64; not to 4; to 4 but not 8; to 8 but not 16
BIG = (1 << 31) - 1
ALL32 = 0xFFFFFFFF
NAN, INF = float("nan"), float("inf")

# symbol -> its arguments after the handle (name, valid default).  A plan call (no handle) is marked by its name.
PAIRS = [("a", P), ("offa", P), ("na", 100), ("b", P), ("offb", P), ("nb", 100), ("n_pairs", 3), ("ratio", 0.8), ("flags", 0),
         ("mab", P), ("mba", None), ("best", None), ("second", None), ("stream", None)]
GUIDED = [("a", P), ("kpa", P), ("offa", P), ("na", 100), ("b", P), ("kpb", P), ("offb", P), ("nb", 100), ("model", P),
          ("n_pairs", 3), ("kind", 0), ("thr", 3.0), ("ratio", 0.8), ("flags", 0), ("mab", P), ("mba", None), ("best", None),
          ("second", None), ("stream", None)]
FLAT = [("a", P), ("na", 64), ("b", P), ("nb", 64), ("lo", None), ("hi", None), ("ratio", 0.8), ("m", P), ("best", None),
        ("second", None), ("stream", None)]
PLAN3 = [("na", 5), ("nb", 5), ("cus", 0), ("o1", None), ("o2", None), ("o3", None)]
VERIFY_DEV = [("kpa", P), ("offa", P), ("kpb", P), ("offb", P), ("m", P), ("n_pairs", 2), ("n_hyp", 256), ("thr", 3.0), ("seed", 0),
              ("flags", 0), ("model", P), ("ver", P), ("stats", P), ("stream", None)]
VERIFY_HOST = [("kpa", P), ("na", 50), ("kpb", P), ("nb", 50), ("m", P), ("n_hyp", 256), ("thr", 3.0), ("seed", 0), ("flags", 0),
               ("model", P), ("ver", P), ("stats", P)]
SIGNATURES = {
    "lf_mkd_match_device": FLAT,
    "lf_mkd_match_both_device": [("a", P), ("na", 64), ("b", P), ("nb", 64), ("ratio", 0.8), ("mab", P), ("mba", P), ("stream", None)],
    "lf_mkd_match": [("a", P), ("na", 64), ("b", P), ("nb", 64), ("ratio", 0.8), ("m", P)],
    "lf_mkd_match_overflowed": [("stream", None), ("n_rows", None)],
    "lf_mkd_match_pairs_device": PAIRS,
    "lf_mkd_match_guided_pairs_device": GUIDED,
    "lf_mkd_quantize_descriptors_device": [("x", P), ("n", 8), ("scale", 256.0), ("q", P), ("stream", None)],
    "lf_mkd_quantize_descriptors": [("x", P), ("n", 8), ("scale", 256.0), ("q", P)],
    "lf_mkd_match_q8_plan": PLAN3,
    "lf_mkd_match_q8_device": FLAT,
    "lf_mkd_match_q8": [("a", P), ("na", 64), ("b", P), ("nb", 64), ("ratio", 0.8), ("m", P)],
    "lf_mkd_knn_q8_plan": [("na", 5), ("nb", 5), ("k", 4), ("cus", 0), ("o1", None), ("o2", None), ("o3", None)],
    "lf_mkd_knn_q8_device": [("a", P), ("na", 64), ("b", P), ("nb", 64), ("lo", None), ("hi", None), ("k", 4), ("index", P),
                             ("score", None), ("stream", None)],
    "lf_mkd_knn_q8": [("a", P), ("na", 64), ("b", P), ("nb", 64), ("k", 4), ("index", P), ("score", None)],
    "lf_mkd_match_q8_grouped_plan": PLAN3,
    "lf_mkd_match_q8_grouped_device": [("a", P), ("na", 64), ("b", P), ("nb", 64), ("group", P), ("lo", None), ("hi", None),
                                       ("ratio", 0.8), ("m", P), ("best", None), ("rival", None), ("stream", None)],
    "lf_mkd_match_q8_grouped": [("a", P), ("na", 64), ("b", P), ("nb", 64), ("group", P), ("ratio", 0.8), ("m", P), ("best", None),
                                ("rival", None)],
    "lf_mkd_vote_groups_device": [("m", P), ("na", 64), ("ga", P), ("n_ga", 4), ("gb", P), ("nb", 64), ("n_gb", 4), ("votes", P),
                                  ("stream", None)],
    "lf_mkd_match_q8_pairs_plan": [("na", 100), ("nb", 100), ("n_pairs", 3), ("both", 0), ("o1", None), ("o2", None)],
    "lf_mkd_match_q8_pairs_device": PAIRS,
    "lf_mkd_match_q8_guided_pairs_device": GUIDED,
    "lf_mkd_edge_layout_device": [("off", P), ("n_images", 4), ("rows", 100), ("edge_image", P), ("n_edges", 3), ("eoff", P),
                                  ("stream", None)],
    "lf_mkd_gather_edge_rows_device": [("src", P), ("row_bytes", 128), ("off", P), ("n_images", 4), ("rows", 100), ("edge_image", P),
                                       ("eoff", P), ("cap", 200), ("n_edges", 3), ("dst", P), ("stream", None)],
    "lf_mkd_match_q8_edges_device": [("a", P), ("offa", P), ("n_ia", 4), ("na", 100), ("b", P), ("offb", P), ("n_ib", 4), ("nb", 100),
                                     ("ea", P), ("eb", P), ("eoa", P), ("ecap_a", 200), ("eob", None), ("ecap_b", 200), ("n_edges", 3),
                                     ("ratio", 0.8), ("flags", 0), ("mab", P), ("mba", None), ("best", None), ("second", None),
                                     ("stream", None)],
    "lf_mkd_build_tracks_device": [("off", P), ("n_images", 4), ("rows", 100), ("ea", P), ("eb", P), ("eoa", P), ("ecap", 200),
                                   ("n_edges", 3), ("m", P), ("flags", 0), ("track", P), ("len", None), ("dup", None), ("stream", None)],
    "lf_mkd_track_table_plan": [("rows", 100), ("min_len", 2), ("o1", None), ("o2", None), ("o3", None), ("o4", None)],
    "lf_mkd_track_table_device": [("off", P), ("n_images", 4), ("rows", 100), ("track", P), ("len", P), ("dup", None), ("min_len", 2),
                                  ("flags", 0), ("tcap", 50), ("ocap", 100), ("toff", P), ("obs_row", P), ("obs_image", P),
                                  ("row_track", None), ("counts", P), ("stream", None)],
    "lf_mkd_gather_track_rows_device": [("src", P), ("row_bytes", 128), ("rows", 100), ("obs_row", P), ("counts", P), ("ocap", 100),
                                        ("dst", P), ("stream", None)],
    "lf_mkd_link_table_plan": [("ecap", 200), ("n_edges", 3), ("o1", None), ("o2", None), ("o3", None), ("o4", None), ("o5", None)],
    "lf_mkd_link_table_device": [("off", P), ("n_images", 4), ("rows", 100), ("ea", P), ("eb", P), ("eoa", P), ("ecap", 200),
                                 ("n_edges", 3), ("m", P), ("min_links", 1), ("flags", 0), ("lcap", 100), ("loff", P), ("la", P),
                                 ("lb", P), ("ledge", None), ("elinks", None), ("kept", None), ("counts", P), ("stream", None)],
    "lf_mkd_select_edges_plan": [("n_a", 8), ("n_b", 8), ("k", 3), ("ecap", 24), ("flags", 0), ("o1", None), ("o2", None), ("o3", None),
                                 ("o4", None), ("o5", None)],
    "lf_mkd_select_edges_device": [("votes", P), ("n_a", 8), ("n_b", 8), ("k", 3), ("min_votes", 1), ("flags", 0), ("ecap", 24),
                                   ("rank", P), ("rank_votes", None), ("ea", P), ("eb", P), ("evotes", None), ("counts", P),
                                   ("stream", None)],
    "lf_mkd_covisibility_plan": [("n_images", 8), ("tcap", 50), ("ocap", 100), ("n_edges", 0), ("flags", 0), ("o1", None), ("o2", None),
                                 ("o3", None), ("o4", None)],
    "lf_mkd_covisibility_device": [("toff", P), ("tcap", 50), ("obs_image", P), ("ocap", 100), ("counts", P), ("n_images", 8),
                                   ("ea", None), ("eb", None), ("n_edges", 0), ("flags", 0), ("covis", P), ("stream", None)],
    "lf_mkd_two_view_pose_device": [("kps", P), ("rows", 100), ("ea", P), ("eb", P), ("n_edges", 3), ("intr", P), ("n_images", 4),
                                    ("F", P), ("loff", P), ("la", P), ("lb", P), ("lcap", 100), ("deg", 1.0), ("flags", 0), ("R", P),
                                    ("t", P), ("stats", P), ("sigma", None), ("points", None), ("stream", None)],
    "lf_mkd_two_view_pose": [("F", P), ("Ka", P), ("Kb", P), ("kpa", P), ("na", 50), ("kpb", P), ("nb", 50), ("m", P), ("deg", 1.0),
                             ("flags", 0), ("R", P), ("t", P), ("stats", P), ("sigma", None), ("points", None)],
    "lf_mkd_triangulate_tracks_device": [("kps", P), ("rows", 100), ("toff", P), ("tcap", 10), ("obs_row", P), ("obs_image", P),
                                         ("ocap", 30), ("counts", P), ("intr", P), ("poses", P), ("n_images", 4), ("px", 4.0),
                                         ("rounds", 2), ("flags", 0), ("points", P), ("stats", P), ("err", None), ("state", None),
                                         ("stream", None)],
    "lf_mkd_triangulate_tracks": [("kps", P), ("rows", 100), ("toff", P), ("n_tracks", 10), ("obs_row", P), ("obs_image", P),
                                  ("n_obs", 30), ("intr", P), ("poses", P), ("n_images", 4), ("px", 4.0), ("rounds", 2), ("flags", 0),
                                  ("points", P), ("stats", P), ("err", None), ("state", None)],
    "lf_mkd_resect_cameras_device": [("kps", P), ("off", P), ("n_images", 4), ("rows", 100), ("rt", P), ("points", P), ("tcap", 10),
                                     ("counts", P), ("intr", P), ("poses", P), ("px", 4.0), ("deg", 0.0), ("n_samples", 64),
                                     ("min_inliers", 12), ("rounds", 3), ("seed", 0), ("flags", 0), ("out", P), ("stats", P),
                                     ("err", None), ("state", None), ("stream", None)],
    "lf_mkd_resect_camera": [("kps", P), ("rows", 100), ("rt", P), ("points", P), ("n_tracks", 10), ("intr", P), ("px", 4.0),
                             ("deg", 0.0), ("n_samples", 64), ("min_inliers", 12), ("rounds", 3), ("seed", 0), ("flags", 0),
                             ("pose", P), ("stats", P), ("err", None), ("state", None)],
    "lf_mkd_verify_homography_device": VERIFY_DEV,
    "lf_mkd_verify_fundamental_device": VERIFY_DEV,
    "lf_mkd_verify_homography": VERIFY_HOST,
    "lf_mkd_verify_fundamental": VERIFY_HOST,
}

# The chains, one row per distinct message in the order the function tests them; {} is the all-valid call ("null handle"), and
# a zero-size row pins "refuse, then early-out".  Where two faults are given together, the earlier check must win.
PAIRS_CASES = [{}, {"n_pairs": 0}, {"a": None}, {"offb": None}, {"mab": None}, {"flags": 2}, {"flags": 2, "a": ODD8}, {"flags": 1},
               {"flags": 1, "mba": P}, {"a": ODD8}, {"b": ODD8, "na": BIG + 1}, {"na": BIG + 1}, {"nb": 1 << 40},
               {"na": BIG, "n_pairs": ALL32}, {"nb": BIG, "n_pairs": ALL32}, {"nb": BIG, "n_pairs": ALL32, "mba": P},
               {"na": BIG, "nb": BIG, "n_pairs": ALL32 >> 1, "mba": P}]
GUIDED_CASES = PAIRS_CASES + [{"kpa": None}, {"kpb": None}, {"model": None}, {"kind": 2}, {"kind": 1}, {"kind": 2, "flags": 2},
                              {"thr": 0.0}, {"thr": NAN}, {"thr": 1e-30}, {"thr": 1e30}, {"thr": 0.0, "kind": 2}, {"thr": 0.0, "a": ODD8},
                              {"thr": 0.0, "n_pairs": 0}]
FLAT_Q8 = [{}, {"na": 0}, {"na": 0, "a": None, "b": None, "m": None}, {"a": None}, {"b": None}, {"m": None}, {"lo": P}, {"hi": P},
           {"lo": P, "hi": P}, {"a": ODD8}, {"b": ODD8}, {"na": 0, "a": ODD8}, {"a": ODD8, "nb": 1}, {"lo": P, "a": ODD8}, {"nb": 1},
           {"nb": 0}, {"na": BIG + 1}, {"nb": 1 << 40}, {"na": 0, "nb": 0}, {"na": BIG, "nb": BIG}]
HOST_Q8 = [{}, {"na": 0}, {"a": None}, {"b": None}, {"m": None}, {"a": ODD2}, {"nb": 1}, {"nb": 0}, {"na": BIG + 1}, {"nb": BIG + 1}]
F32_NULL = [{}, {"na": 0}, {"a": None}, {"nb": 1}]
VERIFY_CASES = [{}, {"n_hyp": 0}, {"n_hyp": 65537}, {"n_hyp": 65536}, {"thr": 0.0}, {"thr": -1.0}, {"thr": NAN}, {"thr": INF},
                {"thr": 1e-30}, {"thr": 1e30}, {"thr": 0.0, "n_hyp": 0}, {"model": None}, {"stats": None}, {"model": None, "n_hyp": 0}]
CASES = [
    ("lf_mkd_match_device", F32_NULL + [{"lo": P}, {"a": ODD8}]),
    ("lf_mkd_match_both_device", F32_NULL + [{"nb": 0}, {"mba": None}]),
    ("lf_mkd_match", F32_NULL),
    ("lf_mkd_match_overflowed", [{}]),
    ("lf_mkd_match_pairs_device", PAIRS_CASES),
    ("lf_mkd_match_guided_pairs_device", GUIDED_CASES),
    ("lf_mkd_quantize_descriptors_device", [{}, {"n": 0}, {"n": 0, "x": None, "q": None}, {"scale": 0.0}, {"x": None}, {"q": None},
                                            {"scale": -1.0}, {"scale": NAN}, {"scale": INF}, {"scale": 1e-40}, {"scale": -1.0, "x": None},
                                            {"n": BIG + 1}, {"n": BIG}, {"x": ODD8}, {"q": ODD2}, {"q": ODD4}, {"n": 0, "x": ODD8},
                                            {"n": BIG + 1, "x": ODD8}]),
    ("lf_mkd_quantize_descriptors", [{}, {"n": 0}, {"scale": 0.0}, {"x": None}, {"q": None}, {"scale": -1.0}, {"scale": 1e-40},
                                     {"n": BIG + 1}, {"x": ODD2, "q": ODD2}]),
    ("lf_mkd_match_q8_plan", [{}, {"na": 0}, {"nb": 1}, {"nb": 0}, {"na": BIG + 1}, {"nb": BIG + 1}, {"na": BIG + 1, "nb": 1},
                              {"na": BIG, "nb": BIG}]),
    ("lf_mkd_match_q8_device", FLAT_Q8),
    ("lf_mkd_match_q8", HOST_Q8),
    ("lf_mkd_knn_q8_plan", [{}, {"k": 0}, {"k": 17}, {"k": 16}, {"k": 1}, {"nb": 0}, {"nb": 1}, {"k": 0, "nb": 0}, {"na": BIG + 1},
                            {"nb": BIG + 1}, {"na": BIG + 1, "nb": 0}]),
    ("lf_mkd_knn_q8_device", [{("index" if k == "m" else k): v for k, v in c.items()} for c in FLAT_Q8] +
     [{"k": 0}, {"k": 17}, {"k": 0, "a": ODD8}, {"k": 0, "nb": 0}, {"k": 0, "lo": P}, {"nb": 1, "k": 16}]),
    ("lf_mkd_knn_q8", [{("index" if k == "m" else k): v for k, v in c.items()} for c in HOST_Q8] + [{"k": 0}, {"k": 17}, {"k": 0, "nb": 0}]),
    ("lf_mkd_match_q8_grouped_plan", [{}, {"na": 0}, {"nb": 1}, {"nb": 0}, {"na": BIG + 1}, {"nb": BIG + 1}, {"na": BIG + 1, "nb": 0}]),
    ("lf_mkd_match_q8_grouped_device", FLAT_Q8 + [{"group": None}, {"group": ODD2}, {"lo": ODD2, "hi": P}, {"lo": P, "hi": ODD2},
                                                  {"m": ODD2}, {"best": ODD2}, {"rival": ODD2}, {"group": ODD2, "a": ODD8},
                                                  {"group": ODD2, "nb": 0}, {"group": ODD2, "na": 0}, {"group": ODD4}]),
    ("lf_mkd_match_q8_grouped", HOST_Q8 + [{"group": None}, {"group": ODD2}]),
    ("lf_mkd_vote_groups_device", [{}, {"na": 0}, {"na": 0, "m": None, "gb": None}, {"m": None}, {"gb": None}, {"ga": None}, {"n_ga": 0},
                                   {"n_gb": 0}, {"n_ga": 0, "m": None}, {"n_ga": 65536, "n_gb": 65536}, {"n_ga": 65536, "n_gb": 32767},
                                   {"votes": None}, {"votes": None, "n_ga": 0}, {"na": BIG + 1}, {"nb": BIG + 1},
                                   {"na": BIG + 1, "votes": None}, {"m": ODD2}, {"ga": ODD2}, {"gb": ODD2}, {"votes": ODD2},
                                   {"m": ODD2, "na": BIG + 1}]),
    ("lf_mkd_match_q8_pairs_plan", [{}, {"n_pairs": 0}, {"na": BIG + 1}, {"nb": BIG + 1}, {"na": BIG, "n_pairs": ALL32},
                                    {"nb": BIG, "n_pairs": ALL32}, {"nb": BIG, "n_pairs": ALL32, "both": 1},
                                    {"na": BIG, "nb": BIG, "n_pairs": ALL32 >> 1, "both": 7}, {"na": BIG, "nb": BIG}]),
    ("lf_mkd_match_q8_pairs_device", PAIRS_CASES),
    ("lf_mkd_match_q8_guided_pairs_device", GUIDED_CASES),
    ("lf_mkd_edge_layout_device", [{}, {"n_edges": 0}, {"n_edges": 0, "off": None, "edge_image": None, "eoff": None}, {"off": None},
                                   {"edge_image": None}, {"eoff": None}, {"off": ODD4}, {"eoff": ODD4}, {"n_edges": 0, "off": ODD4},
                                   {"edge_image": ODD2}, {"edge_image": ODD2, "off": ODD4}, {"rows": BIG + 1}, {"rows": BIG},
                                   {"rows": BIG + 1, "edge_image": ODD2}]),
    ("lf_mkd_gather_edge_rows_device", [{}, {"n_edges": 0}, {"src": None}, {"off": None}, {"edge_image": None}, {"eoff": None},
                                        {"dst": None}, {"n_edges": 0, "dst": None}, {"row_bytes": 0}, {"row_bytes": 516},
                                        {"row_bytes": 130}, {"row_bytes": 4}, {"row_bytes": 512}, {"row_bytes": 0, "src": None},
                                        {"src": ODD2}, {"dst": ODD2}, {"src": ODD2, "row_bytes": 0}, {"rows": BIG + 1}, {"cap": BIG + 1},
                                        {"rows": BIG + 1, "src": ODD2}, {"cap": BIG, "n_edges": ALL32}, {"cap": BIG, "n_edges": BIG}]),
    ("lf_mkd_match_q8_edges_device", [{}, {"n_edges": 0}, {"a": None}, {"offa": None}, {"offb": None}, {"mab": None}, {"ea": None},
                                      {"eb": None}, {"ea": None, "a": None}, {"eoa": None}, {"eoa": None, "ea": None}, {"flags": 2},
                                      {"flags": 2, "eoa": None}, {"flags": 1}, {"flags": 1, "mba": P}, {"mba": P},
                                      {"mba": P, "eob": P}, {"flags": 1, "mba": P, "eob": P}, {"a": ODD8}, {"b": ODD8},
                                      {"a": ODD8, "mba": P}, {"na": BIG + 1}, {"nb": BIG + 1}, {"ecap_a": BIG + 1}, {"ecap_b": BIG + 1},
                                      {"na": BIG + 1, "a": ODD8}, {"ecap_a": BIG, "n_edges": ALL32}, {"ecap_b": BIG, "n_edges": ALL32},
                                      {"ecap_b": BIG, "n_edges": ALL32, "mba": P, "eob": P}, {"n_edges": 0, "flags": 2}]),
    ("lf_mkd_build_tracks_device", [{}, {"rows": 0}, {"n_edges": 0, "ea": None, "eb": None, "eoa": None, "m": None}, {"off": None},
                                    {"track": None}, {"ea": None}, {"eb": None}, {"eoa": None}, {"m": None}, {"ea": None, "eoa": None},
                                    {"eoa": None, "m": None}, {"off": ODD4}, {"eoa": ODD4}, {"off": ODD4, "m": None}, {"ea": ODD2},
                                    {"eb": ODD2}, {"m": ODD2}, {"track": ODD2}, {"len": ODD2}, {"dup": ODD2}, {"ea": ODD2, "off": ODD4},
                                    {"flags": 2}, {"flags": 1}, {"flags": 2, "ea": ODD2}, {"rows": BIG + 1}, {"ecap": BIG + 1},
                                    {"rows": BIG + 1, "flags": 2}, {"ecap": BIG, "n_edges": ALL32}, {"rows": BIG, "n_images": ALL32},
                                    {"rows": BIG, "n_images": ALL32, "dup": P}, {"rows": BIG, "n_images": ALL32, "dup": P, "len": P},
                                    {"rows": 0, "flags": 2}]),
    ("lf_mkd_track_table_plan", [{}, {"min_len": 0}, {"rows": BIG + 1}, {"rows": BIG + 1, "min_len": 0}, {"rows": BIG}, {"rows": 0}]),
    ("lf_mkd_track_table_device", [{}, {"rows": 0}, {"rows": 0, "track": None, "len": None}, {"toff": None}, {"counts": None},
                                   {"track": None}, {"len": None}, {"track": None, "toff": None}, {"obs_row": None},
                                   {"obs_row": None, "ocap": 0}, {"obs_row": None, "track": None}, {"off": None},
                                   {"off": None, "obs_image": None}, {"off": None, "obs_row": None}, {"min_len": 0},
                                   {"min_len": 0, "off": None}, {"flags": 2}, {"flags": 2, "min_len": 0}, {"flags": 1},
                                   {"flags": 1, "dup": P}, {"flags": 1, "rows": 0}, {"flags": 3}, {"off": ODD4}, {"toff": ODD4},
                                   {"off": ODD4, "flags": 1}, {"track": ODD2}, {"len": ODD2}, {"dup": ODD2}, {"obs_row": ODD2},
                                   {"obs_image": ODD2}, {"row_track": ODD2}, {"counts": ODD2}, {"track": ODD2, "toff": ODD4},
                                   {"rows": BIG + 1}, {"tcap": BIG + 1}, {"ocap": BIG + 1}, {"rows": BIG + 1, "track": ODD2},
                                   {"rows": BIG, "tcap": BIG, "ocap": BIG}]),
    ("lf_mkd_gather_track_rows_device", [{}, {"ocap": 0}, {"ocap": 0, "obs_row": None, "dst": None}, {"counts": None}, {"src": None},
                                         {"src": None, "rows": 0}, {"obs_row": None}, {"dst": None}, {"row_bytes": 0},
                                         {"row_bytes": 516}, {"row_bytes": 6}, {"row_bytes": 0, "counts": None}, {"src": ODD2},
                                         {"dst": ODD2}, {"obs_row": ODD2}, {"counts": ODD2}, {"src": ODD2, "row_bytes": 0},
                                         {"rows": BIG + 1}, {"ocap": BIG + 1}, {"rows": BIG + 1, "src": ODD2}, {"ocap": 0, "row_bytes": 0}]),
    ("lf_mkd_link_table_plan", [{}, {"ecap": BIG + 1}, {"ecap": BIG, "n_edges": ALL32}, {"ecap": BIG + 1, "n_edges": ALL32},
                                {"ecap": BIG}, {"ecap": 0, "n_edges": 0}]),
    ("lf_mkd_link_table_device", [{}, {"n_edges": 0, "ea": None, "eb": None, "eoa": None, "m": None}, {"off": None}, {"loff": None},
                                  {"counts": None}, {"ea": None}, {"eb": None}, {"ea": None, "off": None}, {"eoa": None},
                                  {"eoa": None, "ea": None}, {"m": None}, {"m": None, "eoa": None}, {"la": None}, {"lb": None},
                                  {"la": None, "lcap": 0}, {"la": None, "m": None}, {"flags": 2}, {"flags": 1}, {"flags": 2, "la": None},
                                  {"off": ODD4}, {"eoa": ODD4}, {"loff": ODD4}, {"off": ODD4, "flags": 2}, {"ea": ODD2}, {"eb": ODD2},
                                  {"m": ODD2}, {"la": ODD2}, {"lb": ODD2}, {"ledge": ODD2}, {"elinks": ODD2}, {"kept": ODD2},
                                  {"counts": ODD2}, {"ea": ODD2, "off": ODD4}, {"rows": BIG + 1}, {"lcap": BIG + 1},
                                  {"rows": BIG + 1, "ea": ODD2}, {"ecap": BIG + 1}, {"ecap": BIG + 1, "rows": BIG + 1},
                                  {"ecap": BIG, "n_edges": ALL32}]),
    ("lf_mkd_select_edges_plan", [{}, {"k": 0}, {"k": 33}, {"k": 32}, {"flags": 4}, {"flags": 3}, {"flags": 4, "k": 0},
                                  {"flags": 2, "n_b": 9}, {"flags": 2, "n_b": 9, "k": 0}, {"n_b": 0}, {"n_a": 0, "n_b": 0},
                                  {"n_b": 0, "flags": 2}, {"n_a": 65536, "n_b": 65536}, {"n_a": 65536, "n_b": 32767},
                                  {"n_a": ALL32, "n_b": 0}, {"n_a": 1 << 27, "n_b": 1, "k": 32}, {"ecap": BIG + 1},
                                  {"n_a": 65536, "n_b": 65536, "ecap": BIG + 1}]),
    ("lf_mkd_select_edges_device", [{}, {"n_a": 0, "n_b": 0, "votes": None}, {"votes": None}, {"counts": None},
                                    {"counts": None, "votes": None}, {"ea": None}, {"eb": None}, {"ea": None, "ecap": 0},
                                    {"ea": None, "counts": None}, {"votes": ODD2}, {"rank": ODD2}, {"rank_votes": ODD2}, {"ea": ODD2},
                                    {"eb": ODD2}, {"evotes": ODD2}, {"counts": ODD2}, {"votes": ODD2, "ea": None}, {"k": 0},
                                    {"k": 0, "votes": ODD2}, {"flags": 4}, {"flags": 2, "n_b": 9}, {"n_b": 0},
                                    {"n_a": 65536, "n_b": 65536}, {"n_a": 1 << 27, "n_b": 1, "k": 32}, {"ecap": BIG + 1}]),
    ("lf_mkd_covisibility_plan", [{}, {"flags": 2}, {"flags": 1}, {"n_images": 65536}, {"n_images": 46340}, {"n_images": 46341},
                                  {"n_images": 65536, "flags": 2}, {"tcap": BIG + 1}, {"ocap": BIG + 1}, {"tcap": BIG + 1, "n_images": 65536},
                                  {"n_images": 0}]),
    ("lf_mkd_covisibility_device", [{}, {"n_images": 0}, {"n_images": 0, "covis": None}, {"covis": None}, {"counts": None},
                                    {"counts": None, "covis": None}, {"toff": None}, {"toff": None, "counts": None}, {"obs_image": None},
                                    {"obs_image": None, "ocap": 0}, {"obs_image": None, "toff": None}, {"ea": P}, {"eb": P},
                                    {"ea": P, "obs_image": None}, {"n_edges": 3}, {"n_edges": 3, "ea": P, "eb": P}, {"n_edges": 3, "ea": P},
                                    {"toff": ODD4}, {"toff": ODD4, "n_edges": 3}, {"obs_image": ODD2}, {"counts": ODD2},
                                    {"ea": ODD2, "eb": P}, {"ea": P, "eb": ODD2}, {"covis": ODD2}, {"covis": ODD2, "toff": ODD4},
                                    {"flags": 2}, {"flags": 2, "covis": ODD2}, {"n_images": 65536}, {"tcap": BIG + 1}, {"ocap": BIG + 1},
                                    {"n_images": 0, "flags": 2}]),
    ("lf_mkd_two_view_pose_device", [{}, {"n_edges": 0}, {"n_edges": 0, "ea": None, "eb": None, "F": None, "R": None}, {"ea": None},
                                     {"eb": None}, {"F": None}, {"loff": None}, {"R": None}, {"t": None}, {"stats": None},
                                     {"F": None, "ea": None}, {"intr": None}, {"intr": None, "n_images": 0}, {"intr": None, "F": None},
                                     {"la": None}, {"lb": None}, {"la": None, "lcap": 0}, {"la": None, "intr": None}, {"kps": None},
                                     {"kps": None, "rows": 0}, {"kps": None, "lcap": 0}, {"kps": None, "la": None}, {"flags": 1},
                                     {"flags": 1, "kps": None}, {"deg": -0.5}, {"deg": 180.5}, {"deg": NAN}, {"deg": 180.0}, {"deg": 0.0},
                                     {"deg": -0.5, "flags": 1}, {"loff": ODD4}, {"loff": ODD4, "deg": -0.5}, {"kps": ODD2}, {"ea": ODD2},
                                     {"eb": ODD2}, {"intr": ODD2}, {"F": ODD2}, {"la": ODD2}, {"lb": ODD2}, {"R": ODD2}, {"t": ODD2},
                                     {"stats": ODD2}, {"sigma": ODD2}, {"points": ODD2}, {"kps": ODD2, "loff": ODD4}, {"rows": BIG + 1},
                                     {"lcap": BIG + 1}, {"n_edges": BIG + 1}, {"rows": BIG + 1, "kps": ODD2}, {"n_edges": 0, "flags": 1},
                                     {"n_edges": 0, "deg": 181.0}]),
    ("lf_mkd_two_view_pose", [{}, {"na": 0, "nb": 0, "kpa": None, "kpb": None, "m": None}, {"F": None}, {"Ka": None}, {"Kb": None},
                              {"R": None}, {"t": None}, {"stats": None}, {"kpa": None}, {"m": None}, {"kpb": None},
                              {"kpa": None, "F": None}, {"flags": 1}, {"flags": 1, "kpa": None}, {"deg": -0.5}, {"deg": NAN},
                              {"deg": 181.0, "flags": 1}, {"na": BIG + 1}, {"nb": BIG + 1}, {"na": BIG, "nb": 1}, {"na": BIG + 1, "deg": -1.0},
                              {"na": BIG, "nb": 0}]),
    ("lf_mkd_triangulate_tracks_device", [{}, {"tcap": 0}, {"tcap": 0, "toff": None, "counts": None, "points": None, "stats": None},
                                          {"toff": None}, {"counts": None}, {"points": None}, {"stats": None}, {"obs_row": None},
                                          {"obs_image": None}, {"obs_row": None, "ocap": 0}, {"obs_row": None, "toff": None},
                                          {"kps": None}, {"kps": None, "rows": 0}, {"kps": None, "obs_row": None}, {"intr": None},
                                          {"poses": None}, {"intr": None, "n_images": 0}, {"intr": None, "kps": None}, {"flags": 1},
                                          {"flags": 1, "intr": None}, {"px": 0.0}, {"px": -1.0}, {"px": NAN}, {"px": INF},
                                          {"px": 0.0, "flags": 1}, {"rounds": 5}, {"rounds": 4}, {"rounds": 0}, {"rounds": 5, "px": 0.0},
                                          {"toff": ODD4}, {"toff": ODD4, "rounds": 5}, {"kps": ODD2}, {"obs_row": ODD2},
                                          {"obs_image": ODD2}, {"counts": ODD2}, {"intr": ODD2}, {"poses": ODD2}, {"points": ODD2},
                                          {"stats": ODD2}, {"err": ODD2}, {"state": ODD2}, {"kps": ODD2, "toff": ODD4}, {"rows": BIG + 1},
                                          {"tcap": BIG + 1}, {"ocap": BIG + 1}, {"rows": BIG + 1, "kps": ODD2}, {"tcap": 0, "flags": 1},
                                          {"tcap": 0, "rounds": 5}]),
    ("lf_mkd_triangulate_tracks", [{}, {"n_tracks": 0}, {"n_tracks": 0, "toff": None, "points": None, "stats": None}, {"toff": None},
                                   {"points": None}, {"stats": None}, {"obs_row": None}, {"obs_image": None},
                                   {"obs_row": None, "n_obs": 0}, {"kps": None}, {"kps": None, "rows": 0}, {"intr": None}, {"poses": None},
                                   {"intr": None, "n_images": 0}, {"flags": 1}, {"flags": 1, "intr": None}, {"px": 0.0}, {"px": NAN},
                                   {"rounds": 5}, {"rounds": 5, "px": 0.0}, {"rows": BIG + 1}, {"n_tracks": BIG + 1}, {"n_obs": BIG + 1},
                                   {"rows": BIG + 1, "rounds": 5}, {"n_tracks": 0, "rounds": 5}, {"kps": ODD2, "toff": ODD2}]),
    ("lf_mkd_resect_cameras_device", [{}, {"n_images": 0}, {"n_images": 0, "off": None, "counts": None, "intr": None, "poses": None,
                                                            "out": None, "stats": None}, {"off": None}, {"counts": None},
                                      {"intr": None}, {"poses": None}, {"out": None}, {"stats": None}, {"kps": None}, {"rt": None},
                                      {"kps": None, "rows": 0}, {"kps": None, "off": None}, {"points": None}, {"points": None, "tcap": 0},
                                      {"points": None, "kps": None}, {"flags": 2}, {"flags": 1}, {"flags": 2, "points": None}, {"px": 0.0},
                                      {"px": NAN}, {"px": INF}, {"px": 0.0, "flags": 2}, {"deg": -0.5}, {"deg": 180.5}, {"deg": NAN},
                                      {"deg": -0.5, "px": 0.0}, {"n_samples": 0}, {"n_samples": 4097}, {"n_samples": 4096},
                                      {"n_samples": 0, "deg": -0.5}, {"rounds": 5}, {"rounds": 4}, {"rounds": 5, "n_samples": 0},
                                      {"off": ODD4}, {"off": ODD4, "rounds": 5}, {"kps": ODD2}, {"rt": ODD2}, {"points": ODD2},
                                      {"counts": ODD2}, {"intr": ODD2}, {"poses": ODD2}, {"out": ODD2}, {"stats": ODD2}, {"err": ODD2},
                                      {"state": ODD2}, {"kps": ODD2, "off": ODD4}, {"rows": BIG + 1}, {"tcap": BIG + 1},
                                      {"n_images": BIG + 1}, {"rows": BIG + 1, "kps": ODD2}, {"n_images": 0, "flags": 2},
                                      {"n_images": 0, "n_samples": 0}]),
    ("lf_mkd_resect_camera", [{}, {"rows": 0, "kps": None, "rt": None, "points": None}, {"intr": None}, {"pose": None}, {"stats": None},
                              {"kps": None}, {"rt": None}, {"kps": None, "intr": None}, {"points": None}, {"points": None, "n_tracks": 0},
                              {"points": None, "kps": None}, {"flags": 4}, {"flags": 1}, {"flags": 4, "points": None}, {"px": 0.0},
                              {"px": NAN}, {"deg": 181.0}, {"deg": 181.0, "px": 0.0}, {"n_samples": 0}, {"n_samples": 4097}, {"rounds": 5},
                              {"rounds": 5, "n_samples": 0}, {"rows": BIG + 1}, {"n_tracks": BIG + 1}, {"rows": BIG + 1, "rounds": 5},
                              {"kps": ODD2, "pose": ODD2}]),
    ("lf_mkd_verify_homography_device", VERIFY_CASES + [{"n_pairs": 0}, {"n_pairs": 0, "thr": 0.0}, {"kpa": None}, {"offa": None},
                                                        {"kpb": None}, {"offb": None}, {"m": None}, {"ver": None}, {"ver": P, "m": P}]),
    ("lf_mkd_verify_fundamental_device", VERIFY_CASES + [{"n_pairs": 0}, {"n_pairs": 0, "thr": 0.0}, {"kpa": None}, {"ver": None}]),
    ("lf_mkd_verify_homography", VERIFY_CASES + [{"na": 0, "nb": 0, "kpa": None, "kpb": None, "m": None, "ver": None}, {"kpa": None},
                                                 {"m": None}, {"ver": None}, {"kpb": None}, {"kpb": None, "nb": 0}, {"na": BIG + 1}]),
    ("lf_mkd_verify_fundamental", VERIFY_CASES + [{"na": 0, "nb": 0, "kpa": None, "kpb": None, "m": None, "ver": None}, {"kpa": None},
                                                  {"kpb": None}, {"nb": BIG + 1}]),
]


def transcript(L):
    """[{"call", "rc", "message"}] of every case, in order.  The functions that look at the handle first (the f32 matchers)
    return -1 and leave the message alone: their rows repeat the message before them, which is what is pinned."""
    out = []
    assert L.lf_mkd_match_q8_plan(5, 1, 0, None, None, None) == -1     # a known message to begin with, whatever ran before
    for name, cases in CASES:
        assert name in SIGNATURES, name
        sig = SIGNATURES[name]
        fn = getattr(L, name)
        plan = name.endswith("_plan")
        assert len(fn.argtypes) == len(sig) + (0 if plan else 1), name
        for kw in cases:
            assert set(kw) <= {k for k, _ in sig}, (name, kw)
            args = [kw.get(k, v) for k, v in sig]
            rc = fn(*args) if plan else fn(None, *args)
            out.append({"call": "%s %r" % (name, kw), "rc": rc, "message": L.lf_mkd_last_error(None).decode()})
    return out


def _library():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "local-features_amd"))
    import local_features_python as lfp
    return lfp.load_library()         # (LF_MKD_LIB in the environment names another build)


def test_every_symbol_of_the_table_is_driven():
    assert {name for name, _ in CASES} == set(SIGNATURES)
    for name, cases in CASES:
        assert cases[0] == {}, name            # the all-valid call comes first


def test_the_refusals_are_the_recorded_ones():
    want = json.load(open(FIXTURE))
    got = transcript(_library())
    assert [g["call"] for g in got] == [w["call"] for w in want]     # the table and the recording belong together
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, wrong[:5]
    # an all-valid call's only fault is the missing handle, and it says so
    for name, _ in CASES:
        first = next(g for g in got if g["call"] == "%s {}" % name)
        if name.endswith("_plan"):
            assert first["rc"] == 0, first
        elif name in ("lf_mkd_match_device", "lf_mkd_match_both_device", "lf_mkd_match", "lf_mkd_match_overflowed"):
            assert first["rc"] == -1, first
        else:
            assert first["rc"] == -1 and first["message"] == name[len("lf_mkd_"):] + ": null handle", first


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: LF_MKD_LIB=<a library built BEFORE the change under test> test_refusal_transcript.py --record")
    rows = transcript(_library())
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("recorded %d calls to %s" % (len(rows), FIXTURE))
