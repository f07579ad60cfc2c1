"""The rule sets the general exclusion tests use: the shipped config plus four custom regex types and
exclude_info_types rules over them (an allow-list, as a user would write one), and known answers under
them taken from the oracle (literal, not computed)."""
import copy

import xform_configs as X

FULL, PARTIAL = "MATCHING_TYPE_FULL_MATCH", "MATCHING_TYPE_PARTIAL_MATCH"

CUSTOM = [("OUR_DOMAIN", r"@(?:acme|example)\.com"),
          ("TAIL_REF", r"\d{4} ?#\d{3}"),
          ("PAIR3", r"\d{3} \d{3}"),
          ("TEST_CARD", r"4111[ -]?1111[ -]?1111[ -]?1111")]
CUSTOM_NAMES = [n for n, _ in CUSTOM]
BUILTIN_LISTED = ["EMAIL_ADDRESS", "PHONE_NUMBER", "US_SOCIAL_SECURITY_NUMBER", "CREDIT_CARD_NUMBER", "SOCIAL_HANDLE"]


def _types(*names):
    return [{"name": n} for n in names]


def excl_rule(victim: str, excluder: str, matching) -> dict:
    ex = {"exclude_info_types": {"info_types": _types(excluder)}}
    if matching is not None:
        ex["matching_type"] = matching
    return {"info_types": _types(victim), "rules": [{"exclusion_rule": ex}]}


def with_custom(rule_sets, custom=CUSTOM) -> dict:
    """the shipped config (its handle rule kept) + the custom types + these rule sets"""
    cfg = copy.deepcopy(X.shipped())
    insp = cfg["inspect_config"]
    insp["custom_info_types"] = list(insp.get("custom_info_types", [])) + [
        {"info_type": {"name": n}, "regex": {"pattern": p}, "likelihood": "VERY_LIKELY"} for n, p in custom]
    insp["rule_set"] = list(insp.get("rule_set", [])) + list(rule_sets)
    return cfg


G1_RULES = [excl_rule("EMAIL_ADDRESS", "OUR_DOMAIN", PARTIAL),
            excl_rule("PHONE_NUMBER", "TAIL_REF", PARTIAL),
            excl_rule("US_SOCIAL_SECURITY_NUMBER", "PAIR3", PARTIAL),
            excl_rule("CREDIT_CARD_NUMBER", "TEST_CARD", FULL)]
# G2: four excluder patterns beside the shipped one, all FULL_MATCH, no rule on EMAIL_ADDRESS: nothing but
# the number of excluder patterns keeps it from the streaming form
G2_RULES = [excl_rule("SOCIAL_HANDLE", "OUR_DOMAIN", FULL),
            excl_rule("PHONE_NUMBER", "TAIL_REF", FULL),
            excl_rule("US_SOCIAL_SECURITY_NUMBER", "PAIR3", FULL),
            excl_rule("CREDIT_CARD_NUMBER", "TEST_CARD", FULL)]
# G3: G1 as deployed -- the built-in types get their token, the allow-list types are unlisted (kept)
G3_BLOCK = [{"info_types": _types(*BUILTIN_LISTED),
             "primitive_transformation": {"replace_with_info_type_config": {}}}]


def g1() -> dict:
    return with_custom(G1_RULES)


def g1_no_rules() -> dict:
    """G1 with its rule sets removed, the custom types kept (the cost baseline; the shipped rules stay)"""
    return with_custom([])


def g2() -> dict:
    return with_custom(G2_RULES)


def g3() -> dict:
    cfg = g1()
    cfg["deidentify_config"] = {"info_type_transformations": {"transformations": G3_BLOCK}}
    return cfg


def one_more_full() -> dict:
    """the shipped config with one extra FULL_MATCH excluder type: 2 excluder patterns, still streaming"""
    return with_custom([excl_rule("CREDIT_CARD_NUMBER", "TEST_CARD", FULL)], custom=[CUSTOM[3]])


CONFIGS = {"G1": g1, "G2": g2, "G3": g3}

# (row, redacted under G1, redacted under G1 without its rule sets), no context
KNOWN_G1 = [
    # the excluder strictly inside its victim; the excluded e-mail still excludes the handle "@acme.com"
    (b"x jane@acme.com y", b"x jane[OUR_DOMAIN] y", b"x [EMAIL_ADDRESS] y"),
    (b"x jane@acme.org y", b"x [EMAIL_ADDRESS] y", b"x [EMAIL_ADDRESS] y"),
    # the excluder starts before its victim and ends inside it, loses overlap resolution and still excludes
    (b"536-22-1234 #212-555-0187 ok", b"[US_SOCIAL_SECURITY_NUMBER] #212-555-0187 ok",
     b"[US_SOCIAL_SECURITY_NUMBER] #[PHONE_NUMBER] ok"),
    # PAIR3's start at 4 ("222 333") lies inside its previous match: finditer skips it, the SSN stays
    (b"111 222 333-22-4444 ok", b"[PAIR3] [US_SOCIAL_SECURITY_NUMBER] ok", b"[PAIR3] [US_SOCIAL_SECURITY_NUMBER] ok"),
    (b"card 4111 1111 1111 1111 ok", b"card [TEST_CARD] ok", b"card [TEST_CARD] ok"),
]


def write(tmp_dir, name: str, cfg: dict) -> str:
    return X.write(tmp_dir, name, cfg)
