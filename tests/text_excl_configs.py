"""Rule sets for the text exclusion tests: the shipped config plus exclusion_rule.regex, .dictionary and
.exclude_by_hotword rules written the way a user writes an allow-list, chosen against the synth bank
(its e-mail domains, phone prefixes, street names, date forms and the words around card numbers)."""

import excl_configs as XC
import xform_configs as X

FULL, PARTIAL, INVERSE = "MATCHING_TYPE_FULL_MATCH", "MATCHING_TYPE_PARTIAL_MATCH", "MATCHING_TYPE_INVERSE_MATCH"


def _types(*names):
    return [{"name": n} for n in names]


def by_regex(pattern, matching=None) -> dict:
    ex = {"regex": {"pattern": pattern}}
    if matching is not None:
        ex["matching_type"] = matching
    return {"exclusion_rule": ex}


def by_dictionary(words, matching=None) -> dict:
    ex = {"dictionary": {"word_list": {"words": list(words)}}}
    if matching is not None:
        ex["matching_type"] = matching
    return {"exclusion_rule": ex}


def by_hotword(pattern, before=0, after=0) -> dict:
    prox = {}
    if before:
        prox["window_before"] = before
    if after:
        prox["window_after"] = after
    return {"exclusion_rule": {"exclude_by_hotword": {"hotword_regex": {"pattern": pattern}, "proximity": prox}}}


def by_types(excluders, matching=None) -> dict:
    ex = {"exclude_info_types": {"info_types": _types(*excluders)}}
    if matching is not None:
        ex["matching_type"] = matching
    return {"exclusion_rule": ex}


def rule_set(types, *rules) -> dict:
    return {"info_types": _types(*types), "rules": list(rules)}


def with_rules(rule_sets, custom=()) -> dict:
    """the shipped config (its rule sets kept) + custom regex types + these rule sets"""
    return XC.with_custom(rule_sets, custom=list(custom))


# ------------------------------------------------------------------------------------- all forms
# The allow-list of a contact centre, one rule set per concern:
#   - its own mail domains are not PII (regex, PARTIAL: the domain is searched in the address); the
#     dropped address still shields the "@example" handle inside it (the shipped exclude_info_types rule)
#   - phone numbers of the low area codes are its own lines (regex, FULL: the whole number)
#   - only dates written with digits are kept as dates of birth (regex, INVERSE)
#   - addresses in its own streets are its branches (dictionary, PARTIAL, case folded)
#   - numbers said right after "card number", or right before "thanks" / "okay", are test cards read
#     out by staff (exclude_by_hotword, both windows)
ALL_RULES = [
    rule_set(["EMAIL_ADDRESS"], by_regex(r"@(?:example\.com|corp\.test)\b", PARTIAL)),
    rule_set(["PHONE_NUMBER"], by_regex(r"\(?[2-5]\d\d\)?[ .-]\d{3}[ .-]\d{4}")),
    rule_set(["DATE_OF_BIRTH"], by_regex(r"\d\d/\d\d/\d{4}", INVERSE)),
    rule_set(["STREET_ADDRESS"], by_dictionary(["oak", "Maple", "lake view", "Sunset"], PARTIAL)),
    rule_set(["CREDIT_CARD_NUMBER", "FINANCIAL_ACCOUNT_NUMBER", "IMEI_HARDWARE_ID", "DOD_ID_NUMBER"],
             by_hotword(r"(?i)\b(?:card number|thanks|okay)\b", before=24, after=16)),
]


def all_forms() -> dict:
    return with_rules(ALL_RULES)


def all_forms_masked() -> dict:
    """all_forms with a character_mask_config on the card numbers and the shipped token for the rest"""
    cfg = all_forms()
    cfg["deidentify_config"] = {"info_type_transformations": {"transformations": [
        {"info_types": _types("CREDIT_CARD_NUMBER"), "primitive_transformation": X.CARD_MASK},
        {"primitive_transformation": {"replace_with_info_type_config": {}}}]}}
    return cfg


def text_only() -> dict:
    """text exclusion rules and no exclude_info_types rule at all (the shipped handle rule removed): the
    occurrence phases of the general pass have nothing to list"""
    cfg = all_forms()
    for rs in cfg["inspect_config"]["rule_set"]:
        rs["rules"] = [r for r in rs["rules"] if "exclude_info_types" not in r.get("exclusion_rule", {})]
    cfg["inspect_config"]["rule_set"] = [rs for rs in cfg["inspect_config"]["rule_set"] if rs["rules"]]
    return cfg


# ------------------------------------------------------------------------------------- hand-written
# one config for the hand-written rows: custom types with exact shapes, one rule per (form x matching type)
HAND_CUSTOM = [("ORDER_ID", r"ORD-\d{4,8}"),            # regex rules, FULL and PARTIAL
               ("COLOR", r"(?i)\b(?:red|green|blue|teal|dark red)\b"),    # dictionary rules, every matching type
               ("TICKET", r"TK\d{5}"),                  # hotword rule, window_before
               ("BADGE", r"BG\d{4}"),                   # hotword rule, window_after
               ("ZIP9", r"\bz\d{5}-\d{4}"),            # dropped, still excludes ZIP5 (PARTIAL exclude_info_types)
               ("ZIP5", r"\bz\d{5}"),
               ("LONGREF", r"REF [A-Z]{3} \d{6}"),      # dropped: frees the overlapping SHORTREF
               ("SHORTREF", r"[A-Z]{3} \d{6}"),
               ("RUN", r"x?zb+"),                       # finditer: the next start lies inside the dropped match
               ("MARK", r"[#%]")]                       # one-byte quotes
HAND_RULES = [
    # FULL (the default).  The quote's edges are text edges: \b holds at both ends of "ORD-01234" even in "xORD-01234x"
    rule_set(["ORDER_ID"], by_regex(r"\bORD-0\d+\b")),
    rule_set(["ORDER_ID"], by_regex(r"-99", PARTIAL)),
    rule_set(["COLOR"], by_dictionary(["RED"])),                           # FULL, case folded
    rule_set(["COLOR"], by_dictionary(["dark"], PARTIAL)),                 # a word inside the quote
    rule_set(["COLOR"], by_dictionary(["red", "dark red", "green", "blue"], INVERSE)),   # drops "teal"
    rule_set(["TICKET"], by_hotword(r"(?i)\bsample\b", before=12)),
    rule_set(["BADGE"], by_hotword(r"\Avoid\b|\bvoid\Z", after=6)),       # the window's edges are text edges
    rule_set(["ZIP9"], by_regex(r"z00000-\d{4}")),
    rule_set(["ZIP5"], by_types(["ZIP9"], PARTIAL)),
    rule_set(["LONGREF"], by_regex(r"TST", PARTIAL)),
    rule_set(["RUN"], by_regex(r"x.*")),                                   # drops "xzbb"; "zbb" inside it is no match
    rule_set(["MARK"], by_regex(r"#")),
    # INVERSE on a built-in type: only the 800 numbers stay
    rule_set(["PHONE_NUMBER"], by_regex(r"\(?800\)?[ .-]\d{3}[ .-]\d{4}", INVERSE)),
]


def hand() -> dict:
    return with_rules(HAND_RULES, custom=HAND_CUSTOM)


def context_cfg() -> dict:
    """Rules whose effect depends on the row's context variant, on rules/context_variant.json (the rule
    set whose variants differ): IP_ADDRESS is taken out of info_types, so its detector -- and with it the
    rule set's text rule -- exists only under the IP_ADDRESS context group; FINANCIAL_ACCOUNT_NUMBER has
    no hotword rule set there, so its candidates pass min_likelihood only under its own context group
    (the merge appends a '.+' VERY_LIKELY rule set), where the text rule then drops the test accounts."""
    import json
    import os
    from conftest import pkg
    with open(os.path.join(pkg("compiler").RULES_DIR, "context_variant.json")) as f:
        cfg = json.load(f)
    insp = cfg["inspect_config"]
    insp["info_types"] = [t for t in insp["info_types"] if t["name"] != "IP_ADDRESS"]
    insp["rule_set"] = list(insp["rule_set"]) + [
        rule_set(["IP_ADDRESS"], by_regex(r"10\.\d+\.\d+\.\d+")),
        rule_set(["FINANCIAL_ACCOUNT_NUMBER"], by_regex(r"0000\d+")),
        rule_set(["PHONE_NUMBER"], by_hotword(r"(?i)\bfax\b", before=10))]
    return cfg


def write(tmp_dir, name: str, cfg: dict) -> str:
    return X.write(tmp_dir, name, cfg)
