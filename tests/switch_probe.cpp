// Prints every field of the library's switch table as the environment of this process fills it: "member=value", one a line
// (tests/test_switches.py runs it under env= dicts and compares with what the scattered reads it replaces gave).
#include <stdio.h>
#include "a2amd_switches.h"

int main()
{
	A2Switches sw;
	a2amd_read_switches(&sw);
#define X(type, member, read) printf(#member "=%d\n", (int)sw.member);
	A2AMD_SWITCHES(X)
#undef X
	return 0;
}
