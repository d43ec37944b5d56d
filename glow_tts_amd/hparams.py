"""Hyper-parameter loading with the reference's semantics (Arg_Parser.py:3-12, Modules.py:9-13): a yaml file
parsed into nested argparse.Namespace objects.  `get_hp()` reads ./Hyper_Parameters.yaml from the current
working directory (exactly what every reference module does at import time) and falls back to the packaged
defaults; `set_hp()` injects a dict / Namespace (tests, bench)."""
import argparse
import os

import yaml

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_YAML = os.path.join(_HERE, "Hyper_Parameters.default.yaml")
_hp = None


def Recursive_Parse(args_Dict):
    ns = argparse.Namespace()
    for key, value in args_Dict.items():
        setattr(ns, key, Recursive_Parse(value) if isinstance(value, dict) else value)
    return ns


def load_yaml(path):
    with open(path, encoding="utf-8") as f:
        return yaml.load(f, Loader=yaml.Loader)


def set_hp(hp):
    global _hp
    _hp = Recursive_Parse(hp) if isinstance(hp, dict) else hp
    return _hp


def get_hp():
    global _hp
    if _hp is None:
        path = "Hyper_Parameters.yaml" if os.path.exists("Hyper_Parameters.yaml") else DEFAULT_YAML
        _hp = Recursive_Parse(load_yaml(path))
    return _hp


def plain_block(v):
    """A parsed yaml block (nested Namespaces) as plain dicts"""
    return {k: plain_block(x) for k, x in vars(v).items()} if isinstance(v, argparse.Namespace) else v


def overlay_settings(block, defaults, key, noun, rules, also=()):
    """The parsed optional yaml block `block`, named `key` in the yaml, over `defaults` (absent block or key: the default) -> the settings dict of the `noun`
    trainer.  A block that the defaults give as a dict is merged over its default.  An unknown key, at the top level or in such a nested block, raises a
    ValueError naming it; `also` lists sub-blocks the caller reads itself.  `rules(s, need)` states the caller's constraints: need(name, test, allowed) records
    "key.name = value (allowed)" when test(value) is false or raises - a value of the wrong type is a bad value.  All of them leave as ONE ValueError."""
    given = plain_block(block) or {}
    if not isinstance(given, dict):
        raise ValueError(f"{key} must be a mapping, got {given!r}")
    unknown = sorted(set(given) - set(defaults) - set(also))
    if unknown:
        raise ValueError("unknown key {}.{} (known: {})".format(key, unknown[0], ", ".join(defaults)))
    s = dict(defaults, **given)
    for k, d in defaults.items():
        if isinstance(d, dict):
            sub = given.get(k) or {}
            if not isinstance(sub, dict) or set(sub) - set(d):
                raise ValueError("unknown key {}.{}.{} (known: {})".format(key, k, sorted(set(sub) - set(d))[0] if isinstance(sub, dict) else sub, ", ".join(d)))
            s[k] = dict(d, **sub)
    bad = []

    def need(name, test, allowed):
        try:
            good = bool(test(s[name]))
        except (TypeError, ValueError):
            good = False
        if not good:
            v = s[name]
            shown = "{" + ", ".join("{}: {}".format(*kv) for kv in v.items()) + "}" if isinstance(v, dict) else v
            bad.append("{}.{} = {} ({})".format(key, name, shown, allowed))
    rules(s, need)
    if bad:
        raise ValueError("the {} trainer does not support {}".format(noun, "; ".join(bad)))
    return s
