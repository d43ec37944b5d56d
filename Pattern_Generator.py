"""Reference entry point preserved (Pattern_Generator.py:413-545): `python Pattern_Generator.py -lj <path> -vctk <path> -text`; the implementation is
glow_tts_amd/pattern_generator.py."""
from glow_tts_amd.pattern_generator import main  # noqa: F401

if __name__ == "__main__":
    main()
