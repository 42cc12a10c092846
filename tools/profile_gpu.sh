#!/bin/bash
python3 "$(dirname "$0")/profile_record.py" "$@"
